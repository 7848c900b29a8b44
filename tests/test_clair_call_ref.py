"""CPU tests of the restatement tests/clair_call_ref.py itself: the literal pile-up machine against the closed form, the quantize
identity over every `%.6f` text, and the two promotion modes at the ends of p."""
import random

import numpy as np

import clair_call_cases as cc
import clair_call_ref as ref


def test_literal_machine_equals_the_closed_form_on_random_read_sets():
    """up to 600 reads, shared starts, depths around 250: the same reads, in the same order, spelled the same"""
    checked = dropped = 0
    for seed in range(12):
        rng = random.Random(100 + seed)
        n = rng.choice([5, 64, 200, 249, 250, 251, 300, 600])
        starts = sorted(rng.sample(range(60, 130), rng.choice([1, 2, 5, 30])))
        lines = cc.random_reads(seed, n, starts=starts, long_events=seed % 2 == 0)
        reads = [ref.read_of(l) for l in lines]
        for site in rng.sample(range(60, 170), 25):
            literal, closed = ref.literal_sequences(reads, site), ref.closed_sequences(reads, site)
            assert literal == closed, (seed, site)
            everyone = [r for r in ref.overlapping(reads, site) if r[1] <= site - 1 < r[1] + ref.rlen(r[2])]
            dropped += len(everyone) > len(closed)
            checked += 1
    assert checked == 300 and dropped > 0          # the 250 rule did bite, and both forms took the same reads


def test_the_250_rule_takes_other_reads_than_all_overlapping_reads():
    rng = random.Random(3)
    lines = []
    for start, n in ((70, 200), (75, 100), (80, 100)):        # three start groups, 400 reads over the site
        for i in range(n):
            lines.append(cc.line_of(rng, f's{start}.{i}', 0, start, [('M', 30), ('I', 2), ('M', 30)]))
    reads = [ref.read_of(l) for l in lines]
    site = 100
    members = ref.closed_members(reads, site)
    assert [r[1] for r in members] == [70] * 200 + [75] * 50 + [80]          # the first 250, then the first of the next start
    assert len(ref.literal_sequences(reads, site)) == 251 and len(ref.overlapping(reads, site)) == 400


def test_quantize_is_the_text_round_trip_on_all_texts():
    """float32(rint(double(p) * 1e6) / 1e6) against numpy's own parse of 0.000000 .. 1.000000, and idempotent there"""
    q = np.arange(1000001, dtype=np.int64)
    texts = np.char.add(np.char.add((q // 1000000).astype(str), '.'), np.char.zfill((q % 1000000).astype(str), 6))
    parsed = texts.astype(np.float32)
    assert texts[0] == '0.000000' and texts[-1] == '1.000000' and texts[123456] == '0.123456'
    formula = (q.astype(np.float64) / 1e6).astype(np.float32)
    assert parsed.tobytes() == formula.tobytes()
    again = (np.rint(parsed.astype(np.float64) * 1e6) / 1e6).astype(np.float32)
    assert again.tobytes() == parsed.tobytes()
    assert np.array_equal(np.rint(parsed.astype(np.float64) * 1e6).astype(np.int64), q)
    rng = np.random.default_rng(1)
    p = rng.random(20000, dtype=np.float32)
    assert ref.quantize(p).tobytes() == (np.rint(p.astype(np.float64) * 1e6) / 1e6).astype(np.float32).tobytes()


def test_p_one_and_p_zero_in_legacy():
    assert ref.quality(np.float32(1.0), 'legacy') == ref.quality(1.0, 'legacy') > 9000000
    assert ref.quality(np.float32(0.0), 'legacy') == 0
    assert ref.quality(np.float32(0.5), 'legacy') == ref.quality(np.float32(0.5), 'nep50') == 256


def test_the_modes_differ_only_in_quality_and_frequency():
    case = cc.cached_case(11)
    reads = [ref.read_of(l) for l in case['lines']]
    n = 0
    for s, x, p, r in zip(case['sites'], case['x'], case['probs'], case['refs']):
        seqs = ref.closed_sequences(reads, s)
        a = ref.output_with(cc.CTG, s, r, x, p, seqs, cc.fetcher(case['seq']), True, False, True, 100, 'legacy')
        try:
            b = ref.output_with(cc.CTG, s, r, x, p, seqs, cc.fetcher(case['seq']), True, False, True, 100, 'nep50')
        except ValueError:
            assert float(a[1]['p']) == 1.0
            continue
        assert (a is None) == (b is None)
        if a is not None:
            fa, fb = a[0].split('\t'), b[0].split('\t')
            assert fa[:5] == fb[:5] and fa[9].split(':')[0] == fb[9].split(':')[0] and fa[9].split(':')[2] == fb[9].split(':')[2]
            n += 1
    assert n > 50


def test_every_class_and_every_continuation_is_in_the_cases():
    classes, trace = set(), set()
    for seed, all_bases in ((11, True), (12, False), (13, True), (14, False)):
        for got in cc.expected_rows(cc.cached_case(seed, long_events=seed > 12), pysam_all=all_bases, show_ref=True, trace=trace):
            if got is not None:
                flags = got[1]['flags']
                classes.add(flags.index(True))
    assert classes == set(range(10)), classes
    got = cc.expected_rows(cc.reset_case(), pysam_all=True, show_ref=True, trace=trace)
    assert got[0][1]['flags'][0] and got[0][1]['ref'] == got[0][1]['alt']
    assert trace == {'nothing', 'ins_ins reset', 'del_del reset'}, trace


import pytest


@pytest.mark.parametrize('name', cc.GOLDEN_NAMES)
def test_nep50_reproduces_every_golden_byte(name):
    """the reference's own call_var.py under NumPy 2, over the stand-in's literal machine: QUAL and AF included"""
    case = cc.golden_case(name)
    assert cc.golden()['numpy'].startswith('2.')
    reads = [ref.read_of(l) for l in case['lines']]
    kw = case['kw']
    got, legacy = [], []
    for s, x, p, r in zip(case['sites'], case['x'], case['probs'], case['refs']):
        seqs = ref.literal_sequences(reads, s)
        a = ref.output_with(cc.CTG, s, r, x, p, seqs, cc.fetcher(case['seq']), kw['pysam_all'], kw['haploid'], kw['show_ref'], kw['qual'], 'nep50')
        b = ref.output_with(cc.CTG, s, r, x, p, seqs, cc.fetcher(case['seq']), kw['pysam_all'], kw['haploid'], kw['show_ref'], kw['qual'], 'legacy')
        assert (a is None) == (b is None)
        if a is not None:
            got.append(a[0])
            legacy.append(b[0])
    want = cc.records(case['vcf'])
    assert got == want and len(want) > 0
    # REF, ALT, GT and DP of every golden row agree between the modes
    assert [cc.without_float64_columns(l) for l in legacy] == [cc.without_float64_columns(l) for l in want]
