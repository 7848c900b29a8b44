"""CPU tests of the plain restatement the hit stage is checked against (hit_ref.py): it equals the oracle's own gen_regs ->
set_parent -> select_sub -> join_long (exported as mmo_hits_from_chains) hit by hit, field by field and anchor by anchor on every
read of every family of hit_cases.py, it gives the literal values of the hand-worked cases, and the families reach the mechanisms
test_hit_select_gpu.py relies on them to reach (counted by hit_ref's events only, so that a change to the generators cannot
quietly empty a family)."""
import pytest

from hit_cases import COUNTS, HAND, TIE_NAMES, families
from hit_ref import REFUSALS, hit_ref

# what the oracle's mmo_reg holds of a hit (fx .. ly are its first and last anchor in the squeezed list)
ORACLE_KEYS = ('score', 'score0', 'cnt', 'as', 'parent', 'subsc', 'n_sub', 'mlen', 'blen', 'hash', 'sam_pri', 'qs', 'qe', 'rs', 're', 'rid', 'rev', 'id')


@pytest.fixture(scope='module')
def fams():
    return families()


@pytest.fixture(scope='module')
def refs(fams):
    """hit_ref of every read of every batch, computed once and left unchanged: {family: [[(hits, squeezed, ev)]]}"""
    return {name: [[hit_ref(b.k, r.name, r.qlen, *r.u_a(), **b.opt) for r in b.reads] for b in batches] for name, batches in fams.items()}


def oracle_hits(mb, b, r):
    opt = mb.default_opt(**b.opt)
    return mb.hits_from_chains(opt, b.k, r.name, r.qlen, *r.u_a())


def assert_equals_oracle(what, got, want):
    (hits, sq, _), (ohits, osq) = got, want
    assert len(hits) == len(ohits), (what, len(hits), len(ohits))
    for i, (h, o) in enumerate(zip(hits, ohits)):
        for key in ORACLE_KEYS:
            assert h[key] == o['as_' if key == 'as' else key], (what, i, key, h[key], o['as_' if key == 'as' else key])
        if h['cnt'] > 0:
            assert (h['fx'], h['fy'] & ~(1 << 40)) == (int(osq[h['as']][0]), int(osq[h['as']][1]) & ~(1 << 40)), (what, i, 'first anchor')
            assert (h['lx'], h['ly']) == tuple(int(v) for v in osq[h['as'] + h['cnt'] - 1]), (what, i, 'last anchor')
    assert [tuple(int(v) for v in p) for p in osq] == sq, (what, 'squeezed anchors')


def test_ref_equals_oracle_export(oracle_built, fams, refs):
    from oracle import mm2_bindings as mb
    n = 0
    for name, batches in fams.items():
        for b, rs in zip(batches, refs[name]):
            for r, got in zip(b.reads, rs):
                assert_equals_oracle((b.name, r.name), got, oracle_hits(mb, b, r))
                n += 1
    assert n > 800


def test_hand_worked_cases(oracle_built, fams, refs):
    from oracle import mm2_bindings as mb
    assert len(HAND) >= 6
    for (name, opt, qlen, hits, want, want_ev), b, rs in zip(HAND, fams['hand'], refs['hand']):
        got, sq, ev = rs[0]
        orc, _ = oracle_hits(mb, b, b.reads[0])
        for key, vals in want.items():
            assert [h[key] for h in got] == vals, (name, key, [h[key] for h in got], vals)
            assert [o['as_' if key == 'as' else key] for o in orc] == vals, (name, key, 'oracle')
        for key, v in want_ev.items():
            assert ev[key] == v, (name, key, ev[key], v)
    # the five-hit example: a loop that judged every secondary against its own parent would keep hits 0, 2, 3 only
    got = refs['hand'][0][0][0]
    assert [h['score'] for h in got] == [1000, 400, 300, 250]
    by = {name: rs[0] for (name, *_), rs in zip(HAND, refs['hand'])}
    assert sum(1 for x, y in by['join'][1] if y >> 40 & 1) == 1 and by['join'][1][8][1] >> 40 & 1
    assert [i for i, (x, y) in enumerate(by['three-way-join'][1]) if y >> 40 & 1] == [8, 15]
    assert len(by['join-drops-bystander'][1]) == 17          # the bystander's anchors stay in the list its hit has left


def total(rs, key):
    return sum(ev[key] for batch in rs for _, _, ev in batch)


def test_counts_family_sits_on_the_bounds(fams, refs):
    b = fams['counts'][0]
    assert b.max_chains == (0, 3, 48)
    for kind in ('disjoint', 'stacked', 'random'):
        assert sorted(len(r.sorted) for r in b.reads if r.name.startswith(kind)) == sorted(COUNTS)
    for r, (hits, sq, ev) in zip(b.reads, refs['counts'][0]):
        assert len(r.sorted) < 2 or [c.a[0] for c in r.pool] != [c.a[0] for c in r.sorted], r.name
        if r.name.startswith('disjoint'):
            assert len(hits) == len(r.sorted) and all(h['parent'] == i for i, h in enumerate(hits)), r.name
        if r.name.startswith('stacked') and len(r.sorted) > 0:
            assert sum(1 for i, h in enumerate(hits) if h['parent'] == i) == 1 and len(hits) <= 6, r.name
    assert total(refs['counts'][:1], 'drop_best_n') >= 1 and total(refs['counts'][:1], 'kept_2nd') >= 1 and total(refs['counts'][:1], 'hash_ties') >= 1
    # many hits survive under -N 50 -p 0.5: the squeeze and the re-numbering work on long lists
    assert max(len(hits) for hits, _, _ in refs['counts'][1]) > 64


def test_ties_family_is_ordered_by_the_hash(fams, refs):
    for b, rs in zip(fams['ties'], refs['ties']):
        assert total([rs], 'hash_ties') >= 9 * len(b.reads)
        assert {c.a[0][0] >> 63 for r in b.reads for c in r.sorted} == {0, 1}
        kept = {}
        for r, (hits, _, _) in zip(b.reads, rs):
            kept.setdefault((len(r.sorted), r.qlen), {})[r.name] = [h['fx'] for h in hits]
        for (m, qlen), by_name in kept.items():
            if qlen == 2000:     # the same chains under every name: the hash alone picks the primary and the -N survivors
                assert len(by_name) == len(TIE_NAMES) and len({tuple(v) for v in by_name.values()}) >= 2, (b.name, m)
    # ... and under the seeds: the first stack under the first name
    firsts = [rs[0][0] for rs in refs['ties']]
    assert len({tuple(h['fx'] for h in hits) for hits in firsts}) >= 2
    by_q = [[h['fx'] for h in hits] for r, (hits, _, _) in zip(fams['ties'][0].reads, refs['ties'][0]) if len(r.sorted) == 60 and r.name == TIE_NAMES[0]]
    assert len(by_q) == 3 and len({tuple(v) for v in by_q}) >= 2


def test_mask_family_sits_on_the_level(fams, refs):
    for b, rs in zip(fams['mask'], refs['mask']):
        groups = {}
        for r, (hits, _, ev) in zip(b.reads, rs):
            groups.setdefault(r.expect[1], []).append(ev['masked'])
        assert len(groups) >= 12, b.name
        for g, verdicts in groups.items():
            assert len(verdicts) == 4 and len(set(verdicts)) == 2, (b.name, g, verdicts)      # one base decides
        for key in ('masked', 'mask_refused', 'multi_cover', 'triple_cover', 'n_sub_counted', 'n_sub_skipped', 'kept_2nd'):
            assert total([rs], key) >= 2, (b.name, key)
    assert [b.opt['mask_level'] for b in fams['mask']] == [0.5, 0.3]


def test_select_family_reaches_every_verdict(fams, refs):
    seen = set()
    for b, rs in zip(fams['select'], refs['select']):
        p, n = b.opt['pri_ratio'], b.opt['best_n']
        seen.add((p, n))
        ev = {k: total([rs], k) for k in ('kept_2nd', 'drop_ratio', 'drop_best_n', 'drop_identical', 'aliased_parent', 'by_ratio_only', 'by_diff_only', 'resynced')}
        if p == 0:
            assert ev['kept_2nd'] == ev['drop_ratio'] == ev['resynced'] == 0, (b.name, ev)       # the stage is skipped
            assert all(len(hits) == len(r.sorted) for r, (hits, _, _) in zip(b.reads, rs) if not r.name.startswith('alias'))
            continue
        assert ev['kept_2nd'] >= 1 and ev['drop_ratio'] >= 1 and ev['drop_identical'] >= 1, (b.name, ev)
        many = [e for r, (_, _, e) in zip(b.reads, rs) if r.name == 'many'][0]
        assert many['kept_2nd'] == min(n, 60 if p == 0.8 else 30), (b.name, many)
        if n < 30:
            assert many['drop_best_n'] >= 1, b.name
        assert ev['by_ratio_only' if p == 0.8 else 'by_diff_only'] >= 1, (b.name, ev)
        if p == 0.8:
            assert ev['aliased_parent'] >= 1, (b.name, ev)
    assert seen == {(p, n) for p in (0.8, 1.0, 0.0) for n in (1, 5, 50)}
    assert total(refs['select'], 'by_ratio_only') >= 1 and total(refs['select'], 'by_diff_only') >= 1
    # the edges themselves: under -p 0.8 a secondary of (int)(0.8 * s) - 1 goes and one of + 1 stays, whatever the float does at the edge
    b, rs = fams['select'][1], refs['select'][1]
    assert b.opt == dict(pri_ratio=0.8, best_n=5)
    for r, (hits, _, ev) in zip(b.reads, rs):
        if r.name.startswith('edge-') and r.name != 'edge-100':
            s = int(r.name[5:])
            thr = int(round(s * 0.8))
            scores = [h['score'] for h in hits]
            assert thr + 1 in scores and thr - 1 not in scores, (r.name, scores)


def test_join_family_reaches_every_refusal(fams, refs):
    assert fams['join'][0].opt == {} and len(fams['join'][1].opt) == 4
    for b, rs in zip(fams['join'], refs['join']):
        for r, (hits, sq, ev) in zip(b.reads, rs):
            if r.expect is None:
                continue
            kind, what = r.expect
            if kind == 'join':
                assert ev['joins'] == what, (b.name, r.name, ev)
            else:
                assert ev['joins'] == 0 and ev['join_refused_by'][what] >= 1, (b.name, r.name, ev)
        for why in REFUSALS:
            assert sum(ev['join_refused_by'][why] for _, _, ev in rs) >= 2, (b.name, why)
        assert total([rs], 'joins') >= 20 and total([rs], 'chained_joins') >= 6 and total([rs], 'rs_clamped') >= 4
        assert total([rs], 'dropped_by_min_cnt') >= 4
        by = {r.name: x for r, x in zip(b.reads, rs)}
        for sfx in ('', '-rev'):
            # with a join the bystanders below min_cnt go, without one they stay
            assert by['bystanders-join' + sfx][2]['dropped_by_min_cnt'] == 2 and len(by['bystanders-join' + sfx][0]) == 1
            assert by['bystanders-no-join' + sfx][2]['dropped_by_min_cnt'] == 0 and len(by['bystanders-no-join' + sfx][0]) == 4
            for run in (3, 4):
                hits, sq, ev = by['run-%d%s' % (run, sfx)]
                # one hit of all the run's anchors; both secondaries now hang off it (one had the absorbed second hit as its parent)
                assert len(hits) == 3 and hits[0]['cnt'] == 6 * run and [h['parent'] for h in hits] == [0, 0, 0], (run, sfx)
                assert ev['chained_joins'] == run - 2 and sum(1 for x, y in sq if y >> 40 & 1) == run - 1
            assert by['rs-clamp' + sfx][0][0]['rs'] == 0 and by['rs-clamp-single' + sfx][0][0]['rs'] == 0
        # the score threshold: in every sweep some scores join and some do not, on either hit
        sweeps = {}
        for r, (_, _, ev) in zip(b.reads, rs):
            if r.name.startswith('sc-'):
                mg, who = r.name.split('-')[1], r.name.split('-')[2][0]
                sweeps.setdefault((mg, who, r.name.endswith('-rev')), set()).add((ev['joins'], ev['join_refused_by']['sc_thres']))
        assert len(sweeps) == 12 * 2 * 2
        # (all but the gap of 10 under the defaults, where (int)(.5 + .499) = 0 refuses no score)
        two_sided = sum(1 for v in sweeps.values() if v == {(1, 0), (0, 1)})
        assert two_sided >= 44, sorted((k, v) for k, v in sweeps.items() if v != {(1, 0), (0, 1)})
