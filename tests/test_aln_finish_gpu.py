"""GPU tests (-m gpu) of the CIGAR finishing kernel (csrc/fin_kernels.h: gap left-alignment, I/D merging, leading-gap removal,
blen / mlen / n_ambi / dp_max) through its stage entry point mpn_aln_finish_batch, which launches it through the same
fin_enqueue as the mapper.  Every output of every alignment is compared with the sequential restatement of fin_ref.py, exact
integers and exact CIGAR words; test_fin_ref.py pins that restatement to the oracle's fix_cigar / update_extra on the same cases
and asserts that the families of fin_cases.py reach the mechanisms (saturated and dependent gaps, merges, shrinks, leading gaps,
the class bounds) these tests are here for.  force_class runs the small cases through all three LDS classes and global scratch."""
import numpy as np
import pytest

from fin_cases import HAND, LDS_CLASSES, PERIODS, families, on_random
from fin_ref import D, I, KEYS, M, fin_ref, op

pytestmark = pytest.mark.gpu

DEFAULT = dict(a=2, b=4, sc_ambi=1, q_=4, e=2)


@pytest.fixture(scope='module')
def lib(libmpn):
    return libmpn


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    """fin_ref of every case under the default scoring, computed once and left unchanged"""
    return {name: [fin_ref(a.cigar, a.q, a.t) for a in alns] for name, alns in fams.items()}


def run(alns, force_class=0, sc=DEFAULT):
    from megapath_nano_amd import mapper
    opt = mapper.default_opt(a=sc['a'], b=sc['b'], sc_ambi=sc['sc_ambi'], q=sc['q_'], e=sc['e'])
    return mapper.aln_finish_batch(opt, [p.read for p in alns], [(p.qs, p.qe) for p in alns], [p.rev for p in alns], [p.target for p in alns],
                                   [p.ts for p in alns], [p.cigar for p in alns], force_class)


def check(alns, want, what, force_class=0, sc=DEFAULT):
    got = run(alns, force_class, sc)
    assert len(got) == len(alns) == len(want)
    for i, (p, g, w) in enumerate(zip(alns, got, want)):
        for key in KEYS:
            assert g[key] == w[key], (what, 'class %d' % force_class, i, p.name, 'rev' if p.rev else 'fwd', len(p.cigar), key, g[key] if key != 'cigar' else g[key][:24],
                                      w[key] if key != 'cigar' else w[key][:24])
    return got


@pytest.mark.parametrize('period', PERIODS)
def test_repeats_by_op_count(lib, fams, refs, period):
    alns, want = fams['period-%d' % period], refs['period-%d' % period]
    for fc in (0, 1, 4):
        check(alns, want, 'period %d' % period, fc)
    sub = [k for k, a in enumerate(alns) if a.name.endswith('-s0')]
    for fc in (2, 3):
        check([alns[k] for k in sub], [want[k] for k in sub], 'period %d' % period, fc)


@pytest.mark.parametrize('family', ['leading', 'merge', 'zero_span', 'hand'])
def test_constructed_cases(lib, fams, refs, family):
    for fc in (0, 1, 2, 3, 4):
        got = check(fams[family], refs[family], family, fc)
        if family == 'leading':    # the statistics come from the shifted offsets: a leading gap's bases are in none of them
            for p, g in zip(fams[family], got):
                if p.name.startswith('lead-'):
                    assert g['qshift'] + g['tshift'] > 0, p.name
                    qn = sum(c >> 4 for c in g['cigar'] if c & 15 != D)
                    tn = sum(c >> 4 for c in g['cigar'] if c & 15 != I)
                    assert qn == len(p.q) - g['qshift'] and tn == len(p.t) - g['tshift'], p.name
        if family == 'hand':
            for (name, _, _, _, literal), g in zip(HAND, got):
                assert {k: g[k] for k in KEYS} == literal, (name, fc)


def test_word_and_strand_offsets(lib, fams, refs):
    """every offset of the first and last aligned read base in its 4-byte word on both strands, every offset of the first target
    base in its 2-bit word; the first pair reads below the reads buffer, the last one ends in the last packed word"""
    offs = fams['offsets']
    assert offs[0].rev == 1 and offs[0].qs == 0 and offs[-1].ts + len(offs[-1].t) == len(offs[-1].target)
    for fc in (0, 4):
        check(offs, refs['offsets'], 'offsets', fc)


def test_ambiguous_bases(lib, fams, refs):
    alns = fams['ambiguous']
    assert any(r['n_ambi'] > 0 for r in refs['ambiguous'])
    for sc_ambi in (0, 1, 3):
        sc = dict(DEFAULT, sc_ambi=sc_ambi)
        want = refs['ambiguous'] if sc_ambi == 1 else [fin_ref(a.cigar, a.q, a.t, **sc) for a in alns]
        for fc in (0, 4):
            check(alns, want, 'N, sc_ambi %d' % sc_ambi, fc, sc)


def scoring_sets():
    from test_ext_scoring_gpu import SETS
    from test_map_e2e_gpu import SCORING_SETS
    out = {'default': DEFAULT}
    for src, sets in (('ext', SETS), ('e2e', SCORING_SETS)):
        for name, s in sets.items():
            out[src + '-' + name] = dict(a=s['a'], b=s['b'], sc_ambi=s.get('sc_ambi', 1), q_=s['q'], e=s['e'])
    return out


def test_dp_max_under_scoring_sets(lib, fams, refs):
    alns = fams['dpmax'] + [a for a in fams['period-2'] if a.name.endswith('-s1')]
    sets = scoring_sets()
    assert len(sets) > 15
    seen = set()
    for name, sc in sets.items():
        want = [fin_ref(a.cigar, a.q, a.t, **sc) for a in alns]
        seen |= {w['dp_max'] for w in want}
        check(alns, want, 'dp_max, ' + name, 0, sc)
        if name in ('default', 'ext-asm5', 'ext-A15'):
            check(alns, want, 'dp_max, ' + name, 4, sc)
    assert 0 in seen and len(seen) > 50


def test_size_classes_in_one_batch(lib, fams, refs):
    """needs of exactly 16384 / 16388 / 32768 / 32772 / 65536 / 65540 bytes (the last LDS byte of a class and the first of the next)
    and five alignments in global scratch, interleaved with small ones: the launch lists reorder the jobs, and the scratch offsets
    of the global path go by list position"""
    alns = fams['sizes']
    needs = [a.need for a in alns]
    assert all(needs.count(x) == 2 and needs.count(x + 4) == 2 for x in LDS_CLASSES) and sum(1 for x in needs if x > LDS_CLASSES[-1]) >= 5
    check(alns, refs['sizes'], 'size classes', 0)


def test_batch_invariance(lib, fams, refs):
    alns = fams['merge'][:6] + fams['period-1'][::4] + fams['leading'][:4] + [a for a in fams['sizes'] if a.need > LDS_CLASSES[-1]][:2]
    want = [fin_ref(a.cigar, a.q, a.t) for a in alns]
    whole = check(alns, want, 'one call')
    rev = check(alns[::-1], want[::-1], 'reversed')
    assert rev[::-1] == whole
    for k in range(0, len(alns), 3):
        assert check([alns[k]], [want[k]], 'alone') == [whole[k]]


def test_refusals(lib, fams):
    from megapath_nano_amd import _ffi
    rng = np.random.default_rng(9)
    good = on_random(rng, 'good', [op(30, M), op(2, I), op(30, M)])
    assert run([good])[0]['n_cigar'] == 3
    for bad_cigar in ([op(30, M), op(2, I), op(29, M)],      # does not consume its read interval
                      [op(30, M), op(2, I), op(31, M)],
                      [op(62, 4)],                           # a soft clip: not M / I / D
                      [op(30, M), op(2, 3), op(30, M)],
                      [op(30, M), op(2, I), op(30, M), op(50, D)]):   # leaves the target
        bad = on_random(rng, 'bad', [op(30, M), op(2, I), op(30, M)])
        bad.cigar = bad_cigar
        with pytest.raises(_ffi.MpnError, match=r'rc=-1'):
            run([good, bad])
    by_need = {a.need: a for a in fams['sizes']}
    for fc, lds in zip((1, 2, 3), LDS_CLASSES):
        with pytest.raises(_ffi.MpnError, match=r'rc=-1'):
            run([good, by_need[lds + 4]], fc)
        assert run([good, by_need[lds]], fc)[0]['n_cigar'] == 3
    with pytest.raises(_ffi.MpnError, match=r'rc=-1'):
        run([good], 5)
    # an alignment without ops is not launched and returns zeros
    empty = on_random(rng, 'no-ops', [], ql=4, tl=4)
    assert run([empty, good, empty])[0] == dict(n_cigar=0, qshift=0, tshift=0, blen=0, mlen=0, n_ambi=0, dp_max=0, cigar=[])
