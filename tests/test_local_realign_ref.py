"""CPU tests of the restatement tests/local_realign_ref.py against the goldens that the reference's own programs wrote
(tests/golden/make_local_realign_golden.py: the real mpileup, local_realignment.py, extract_vcf_position.py)."""
import random
import re

import pytest

import local_realign_cases as lc
import local_realign_ref as ref

pytestmark = pytest.mark.usefixtures('oracle_built')


@pytest.mark.parametrize('case', lc.golden_cases(), ids=lambda c: c['name'])
def test_lines_equal_the_goldens(case):
    assert not case['raised']
    assert ref.lines(lc.reads_of(case), case['seq'], lc.CTG, case['positions']) == case['expected_lines']


@pytest.mark.parametrize('case', lc.golden_cases(), ids=lambda c: c['name'])
def test_vcf_equals_the_goldens(case):
    vcf, said = ref.extract_vcf_position(case['vcf'], case['expected_lines'])
    assert vcf == case['expected_vcf'] and said == case['expected_stdout']
    assert not vcf.endswith('\n')


def test_the_goldens_update_and_keep_rows():
    snp = next(c for c in lc.golden_cases() if c['name'] == 'snp')
    rows = [r for r in snp['expected_vcf'].splitlines() if r[0] != '#']
    before = [r for r in snp['vcf'].splitlines() if r[0] != '#']
    assert len(rows) == 3 and rows[0] == rows[2] != before[0] and rows[1] == before[1]      # the duplicate position twice; no SNP: unchanged
    assert snp['expected_stdout'].count('[INFO]') == 2


def test_a_golden_read_has_a_leading_ssw_clip_and_a_site_stops_after_the_centre():
    clipped = stopped = 0
    for case in lc.golden_cases():
        reads = lc.reads_of(case)
        for pos in case['positions']:
            detail = []
            ref.site(reads, case['seq'], pos, detail=detail)
            clipped += sum(1 for f, res in detail if res[0] > 0 and res[4] > 0)
            acc = ref.members(reads, pos)
            cols = ref.window(reads, acc, pos)
            hi = cols[-1] if cols else pos
            later = any(hi + 1 < reads[i][1] + 1 <= pos + ref.WINDOW and not ref.refuse(reads[i]) for i in acc)
            stopped += hi < pos + ref.WINDOW and later
    assert clipped > 0 and stopped > 0


@pytest.mark.parametrize('seed', range(6))
def test_the_depth_rule_equals_the_machine_with_a_small_maxcnt(seed):
    rng = random.Random(seed)
    seq = lc.pc.random_contig(rng, 1400)
    lines = []
    for i in range(60):
        s = rng.choice([480, 480, 500, 500, 500, 530, 600, 640])
        lines.append(lc.span_read(rng, seq, f'd{i}', s, f'{rng.choice([20, 60, 150, 300])}M'))
    lines.sort(key=lambda l: int(l.split('\t')[3]))
    reads = [ref.ccr.read_of(l) for l in lines]
    for maxcnt in (3, 4, 5, 6):
        plp = ref.ccr.Pileup([r for r in reads if r[1] < 700 + ref.REGION + 1 and r[1] + ref.ccr.rlen(r[2]) > 700 - ref.REGION - 1], maxcnt=maxcnt)
        while plp.auto() is not None:
            pass
        machine = [id(r) for r in plp.pushed]
        closed = [id(reads[i]) for i in ref.members(reads, 700, maxcnt)]
        assert closed == machine and len(closed) < len(reads)


_SSW = {}


def cached_ssw(query, window):
    if (query, window) not in _SSW:
        _SSW[(query, window)] = ref.oracle_ssw(query, window)
    return _SSW[(query, window)]


def test_the_deep_golden_where_the_real_depth_rule_acts():
    """11200 reads over eight starts: mpileup's -d 8000 drops some, and the closed form drops the same ones"""
    case = lc.deep_golden()
    reads = lc.reads_of(case)
    kept = len(ref.members(reads, case['positions'][0]))
    assert len(reads) > kept >= 8000
    assert ref.lines(reads, case['seq'], lc.CTG, case['positions'], ssw=cached_ssw) == case['expected_lines']
    assert ref.lines(reads, case['seq'], lc.CTG, case['positions'], ssw=cached_ssw, maxcnt=1 << 30) != case['expected_lines']
    assert ref.extract_vcf_position(case['vcf'], case['expected_lines']) == (case['expected_vcf'], case['expected_stdout'])


# ---- the literal form (mpileup's text through the script's parse) against the closed form ----------------------------------------------
def random_cigar(rng, span):
    """operations over about `span` reference bases: clips, a leading insertion, insertions, deletions, an insertion right before and
    right behind a deletion, two insertions in a row"""
    ops = []
    if rng.random() < 0.3:
        ops.append((rng.choice('SH'), rng.randrange(1, 6)))
    if rng.random() < 0.2:
        ops.append(('I', rng.randrange(1, 4)))
    left = span
    while left > 0:
        n = min(left, rng.randrange(1, 60))
        ops.append((rng.choice('M=X'), n))
        left -= n
        if left <= 0:
            break
        kind = rng.random()
        if kind < 0.25:
            ops.append(('I', rng.randrange(1, 5)))
        elif kind < 0.5:
            d = rng.randrange(1, 12)
            ops.append(('D', d))
            left -= d
        elif kind < 0.6:
            ops += [('I', rng.randrange(1, 4)), ('D', rng.randrange(1, 4))]
        elif kind < 0.7:
            ops += [('D', rng.randrange(1, 4)), ('I', rng.randrange(1, 4))]
        elif kind < 0.8:
            ops += [('I', 2), ('I', 1)]
    if ops[-1][0] == 'D' or (ops[-1][0] == 'I' and ops[-2][0] == 'D'):
        ops.append(('M', 3))
    if rng.random() < 0.2:
        ops.append(('I', 2))
    if rng.random() < 0.3:
        ops.append(('S', rng.randrange(1, 6)))
    return ''.join('%d%s' % (n, op) for op, n in ops)


def random_set(seed):
    """reads in two clusters with a gap between them on some seeds, few starts (so that a small maxcnt bites), both strands, flags that
    are and are not piled up, N and IUPAC bases"""
    rng = random.Random(seed)
    seq = lc.pc.random_contig(rng, 1500)
    starts = [rng.randrange(430, 700) for _ in range(6)] + [rng.randrange(700, 930) for _ in range(3)]
    lines = []
    for i in range(50):
        s = rng.choice(starts)
        flag = rng.choice([0, 0, 0, 16, 16, 2048, 2064, 256, 1024])
        lines.append(lc.span_read(rng, seq, f'q{i}', s, random_cigar(rng, rng.choice([15, 40, 90, 200, 320])), flag=flag, sub=rng.choice([0, 0.01, 0.05])))
    lines.sort(key=lambda l: int(l.split('\t')[3]))
    return seq, [ref.ccr.read_of(l) for l in lines]


def both(reads, pos, maxcnt):
    """closed and literal fragments; None where the script raises"""
    out = []
    for f in (ref.fragments_of, ref.literal_fragments_of):
        try:
            out.append(f(reads, pos, maxcnt))
        except ref.SiteRaises:
            out.append(None)
    return out


@pytest.mark.parametrize('seed', range(12))
def test_literal_and_closed_form_agree_on_random_read_sets(seed):
    """fragments and dict order for maxcnt 3 .. 6 and 8000; the lines for one lowered maxcnt"""
    seq, reads = random_set(100 + seed)
    for pos in (700, 640, 790):
        for maxcnt in (3, 4, 5, 6, ref.MAXCNT):
            closed, literal = both(reads, pos, maxcnt)
            assert closed == literal, (pos, maxcnt)
    maxcnt = 3 + seed % 4
    assert ref.lines(reads, seq, lc.CTG, [700, 640, 790], ssw=cached_ssw, maxcnt=maxcnt) == \
        ref.lines(reads, seq, lc.CTG, [700, 640, 790], ssw=cached_ssw, maxcnt=maxcnt, literal=True)


def test_the_random_sets_hold_what_they_are_for():
    """dropped rows, `+ins-del`, leading insertions, a stop behind the centre, a raising parser, a biting depth rule: each occurs"""
    rows = drops = insdel = stops = lead = raised = bites = 0
    for seed in range(12):
        seq, reads = random_set(100 + seed)
        bites += len(ref.members(reads, 700, 3)) < len(ref.members(reads, 700))
        text = ref.mpileup_text(reads, 700)
        raised += sum(both(reads, pos, m)[1] is None for pos in (700, 640, 790) for m in (3, ref.MAXCNT))
        try:
            table = ref.parse_pileup(text)
        except IndexError:
            continue
        rows += text.count('\n')
        drops += text.count('\n') - len(table)
        insdel += sum(1 for r in text.splitlines() if re.search(r'\+\d+[A-Za-z]+-\d+', r.split('\t')[4]))
        stops += any(p not in table for p in range(701, 901)) and any(p in table for p in range(701, 901))
        lead += sum(1 for r in reads if [op for op, n in r[2] if op not in 'SH'][0] == 'I')
    assert drops > 0 and insdel > 0 and stops > 0 and lead > 0 and rows > 3000 and raised > 0 and bites == 12


@pytest.mark.parametrize('case', lc.golden_cases(), ids=lambda c: c['name'])
def test_the_literal_form_reproduces_the_goldens(case):
    reads = lc.reads_of(case)
    assert ref.lines(reads, case['seq'], lc.CTG, case['positions'], ssw=cached_ssw, literal=True) == case['expected_lines']
    for pos in case['positions']:
        assert ref.fragments_of(reads, pos) == ref.literal_fragments_of(reads, pos)
