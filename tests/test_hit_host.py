"""CPU test: the mapper's host hit path (csrc/hit_host.cpp: gen_regs, set_parent, select_sub, squeeze_a, join_long -- the only path
of reads with more than 384 chains) and the hits accumulator's block format (csrc/hits_block.cpp: what ranks send each other) built
for the host with g++ (scripts/hit_host_check.cpp, under AddressSanitizer and UBSan where the toolchain has their runtimes), against
the restatement tests/hit_ref.py: every read of every family of hit_cases.py with the batch's own options, with and without
CIGARs, every hit field and every squeezed anchor as exact integers; and blocks of those hits exported, imported and offered to
the importer truncated at every length and with every single-byte change."""
import struct

import pytest

import hit_cases as hc
from hit_ref import KEYS, hit_ref


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return hc.build_host_check(tmp_path_factory.mktemp('hit_host'))


@pytest.fixture(scope='module')
def fams():
    return hc.families()


@pytest.fixture(scope='module')
def refs(fams):
    """hit_ref of every read of every batch, computed once and left unchanged"""
    return {name: [[hit_ref(b.k, r.name, r.qlen, *r.u_a(), **b.opt) for r in b.reads] for b in batches] for name, batches in fams.items()}


def opt_bytes(b, with_cigar):
    from megapath_nano_amd import mapper
    return bytes(mapper.default_opt(with_cigar=with_cigar, **b.opt))


def test_every_read_of_every_family_equals_the_restatement(exe, tmp_path, fams, refs):
    compared = 0
    for with_cigar in (1, 0):
        batches = [b for name in fams for b in fams[name]]
        wants = [w for name in fams for w in refs[name]]
        got = hc.host_hits(exe, tmp_path, [(b, opt_bytes(b, with_cigar)) for b in batches])
        assert len(got) == len(batches)
        for b, want, reads in zip(batches, wants, got):
            assert len(reads) == len(b.reads) == len(want)
            for r, (whits, wsq, _), (hits, n_a, segs) in zip(b.reads, want, reads):
                what = (b.name, r.name, len(r.pool), 'with_cigar %d' % with_cigar)
                assert len(hits) == len(whits) and n_a == len(wsq), what
                for i, (h, w) in enumerate(zip(hits, whits)):
                    for key in KEYS:
                        assert h[key] == w[key], what + ('hit %d' % i, key, h[key], w[key])
                if with_cigar:
                    assert hc.squeezed(r, n_a, segs) == wsq, what
                else:
                    assert segs == []
                compared += 1
    n_reads = sum(len(b.reads) for batches in fams.values() for b in batches)
    assert n_reads > 800 and compared == 2 * n_reads                     # no read skipped
    assert max(len(r.pool) for b in fams['counts'] for r in b.reads) > 384   # the reads the kernel leaves to the host are among them


def block_reads(fams, refs, with_cigar):
    """a few reads' hits as the block carries them: a hand-worked join, a stack of tied secondaries, a read without hits"""
    picked = [(fams['hand'][1].reads[0], refs['hand'][1][0]), (fams['ties'][0].reads[0], refs['ties'][0][0]), (fams['counts'][0].reads[0], [[], [], None]),
              (fams['hand'][0].reads[0], refs['hand'][0][0])]
    reads = []
    for n, (r, (hits, _, _)) in enumerate(picked):
        rows = []
        for i, h in enumerate(hits[:2]):
            has_p = 1 if with_cigar else 0
            f = dict(h, inv=0, split=i & 1, hash=h['hash'] - (1 << 32) if h['hash'] >> 31 else h['hash'], has_p=has_p, dp_score=has_p * (h['score'] + 7),
                     dp_max=has_p * (h['score'] + 9), n_ambi=has_p * i)
            cig = [(h['qe'] - h['qs']) << 4, 3 << 4 | 1 + (i & 1), 5 << 4] if with_cigar and i == 0 else []
            rows.append((tuple(f[key] for key in hc.BLOCK_FIELDS), tuple(cig)))
        reads.append((100 * n + 1, rows))
    return reads


@pytest.mark.parametrize('want_text', [1, 0])
@pytest.mark.parametrize('with_cigar', [1, 0])
def test_a_block_round_trips_and_no_damaged_block_is_taken(exe, tmp_path, fams, refs, with_cigar, want_text):
    reads = block_reads(fams, refs, with_cigar)
    assert sum(len(h) for _, h in reads) >= 5 and any(not h for _, h in reads[1:3])
    lens = [100000 + t for t in range(1 + max(f[1] for _, hits in reads for f, _ in hits))]
    lo, hi = 1, 3                                                        # a sub-range: a read with hits and one without
    size, (k, n_parts, lens2, got), counts = hc.host_block(exe, tmp_path, 15, want_text, 2, lens, reads, lo, hi)
    payload = sum(8 + sum(72 + (4 + 4 * len(cig) if want_text else 0) for _, cig in hits) for _, hits in reads[lo:hi])
    assert size == 48 + payload and size < 1000
    # what the format carries, after two imports: the second import's hits behind the first's, their targets behind its targets
    assert (k, n_parts, lens2) == (15, 4, lens + lens)
    for (rep_len, hits), (rep2, hits2) in zip(reads[lo:hi], got):
        assert rep2 == rep_len and len(hits2) == 2 * len(hits)
        for shift, part in ((0, hits2[:len(hits)]), (len(lens), hits2[len(hits):])):
            for (f, cig), (f2, cig2) in zip(hits, part):
                want = list(f)
                want[1] += shift
                assert list(f2) == want and tuple(cig2) == (tuple(cig) if want_text else ())
    n_trunc, n_payload, n_check, n_head_ok, n_head_no = counts
    assert n_trunc == size                                              # every length 0 .. size - 1 refused
    assert n_payload == 255 * payload and n_check == 255 * 8             # every other value of every payload and check byte refused
    assert n_head_ok + n_head_no == 255 * 40 and n_head_ok <= 255 * 8    # the rest of the header: free are the pad word, and k for an empty accumulator
    assert struct.calcsize('<4sI6iqQ') == 48
