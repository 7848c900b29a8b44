"""GPU tests (-m gpu) of the difference-string kernel (csrc/tag_kernels.h) through its stage entry point mpn_aln_tags_batch:
cs (short and long form), MD and the =/X CIGAR of synthetic alignments against the plain-Python writer of diff_tags_ref.py,
byte for byte.  The shapes are the smallest at which the kernel can go wrong: chunk boundaries of 64 columns, digit-count
boundaries of the run counts, events next to each other, every word offset of the read and of the 2-bit target on both strands,
CIGARs on both sides of the LDS classes (512 and 4096 ops) and one alignment that leaves them."""
import numpy as np
import pytest

from diff_tags_ref import CS, CS_LONG, EQX, MD, MD_RE, collapse_eqx, revcomp_codes, write_tags

pytestmark = pytest.mark.gpu

M, I, D = 0, 1, 2


def op(n, o):
    return n << 4 | o


class Pair:
    """One alignment: q (codes, alignment orientation) against t under cigar; placed in a read with flanks (read orientation:
    for rev the reverse complement of q sits between them) and in a target with flanks."""

    def __init__(self, cigar, q, t, rev=0, ql=0, qr=0, tl=0, tr=0, rng=None):
        rng = rng or np.random.default_rng(len(q) * 7 + len(t))
        self.cigar, self.q, self.t, self.rev = list(cigar), np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8), rev
        mid = revcomp_codes(self.q) if rev else self.q
        self.read = np.concatenate([rng.integers(0, 4, ql), mid, rng.integers(0, 4, qr)]).astype(np.uint8)
        self.qs, self.qe = ql, ql + len(self.q)
        self.target = np.concatenate([rng.integers(0, 4, tl), self.t, rng.integers(0, 4, tr)]).astype(np.uint8)
        self.ts = tl


def from_cigar(rng, cigar, mismatch_cols=(), **kw):
    """random target; the read equals it in every M column but those of mismatch_cols (indices among ALL columns)"""
    tspan = sum(c >> 4 for c in cigar if c & 15 != I)
    t = rng.integers(0, 4, tspan).astype(np.uint8)
    q, ti, col, mm = [], 0, 0, set(mismatch_cols)
    for c in cigar:
        ln, o = c >> 4, c & 15
        for _ in range(ln):
            if o == M:
                q.append((int(t[ti]) + 1 + int(rng.integers(0, 3))) % 4 if col in mm else int(t[ti]))
                ti += 1
            elif o == I:
                q.append(int(rng.integers(0, 4)))
            else:
                ti += 1
            col += 1
    return Pair(cigar, q, t, rng=rng, **kw)


def random_pair(rng, length, err, **kw):
    """an alignment of about `length` columns with error rate err (a third each substitutions, insertions, deletions)"""
    kinds = rng.choice(4, size=length, p=[1 - err, err / 3, err / 3, err / 3])   # match, mismatch, insertion, deletion
    q, t, cigar = [], [], []
    for k in kinds:
        o = M if k < 2 else I if k == 2 else D
        if o != I:
            t.append(int(rng.integers(0, 4)))
        if o == M:
            q.append(t[-1] if k == 0 else (t[-1] + 1 + int(rng.integers(0, 3))) % 4)
        elif o == I:
            q.append(int(rng.integers(0, 4)))
        if cigar and cigar[-1] & 15 == o:
            cigar[-1] += 16
        else:
            cigar.append(op(1, o))
    return Pair(cigar, q, t, rng=rng, **kw)


def run(pairs, tags, caps=None):
    from megapath_nano_amd import mapper
    return mapper.aln_tags_batch([p.read for p in pairs], [(p.qs, p.qe) for p in pairs], [p.rev for p in pairs],
                                 [p.target for p in pairs], [p.ts for p in pairs], [p.cigar for p in pairs], tags, caps)


def check(pairs, what):
    """both calls (short cs + MD + =/X, then long cs) against the writer; -> the first call's results"""
    got = run(pairs, CS | MD | EQX)
    got_long = run(pairs, CS_LONG)
    assert len(got) == len(got_long) == len(pairs)
    for i, (p, g, gl) in enumerate(zip(pairs, got, got_long)):
        want = write_tags(p.cigar, p.q, p.t)
        tag = (what, i, 'rev' if p.rev else 'fwd', len(p.cigar))
        assert g['cs'] == want['cs'], tag + ('cs', g['cs'][:200], want['cs'][:200])
        assert g['md'] == want['md'], tag + ('MD', g['md'][:200], want['md'][:200])
        assert g['eqx'] == want['eqx'], tag + ('eqx', g['eqx'][:40], want['eqx'][:40])
        assert gl['cs'] == want['cs_long'], tag + ('cs long', gl['cs'][:200], want['cs_long'][:200])
        assert gl['md'] is None and gl['eqx'] is None
        assert collapse_eqx(g['eqx']) == collapse_eqx(p.cigar), tag
        assert not p.cigar or MD_RE.match(g['md']), tag
    return got


@pytest.fixture(scope='module')
def lib(libmpn):
    return libmpn


def test_length_boundaries(lib):
    rng = np.random.default_rng(1)
    pairs = []
    for n in (1, 63, 64, 65, 127, 128, 129):
        pairs.append(from_cigar(rng, [op(n, M)]))
        for col in (0, 63, 64, n - 1):
            if col < n:
                pairs.append(from_cigar(rng, [op(n, M)], [col], rev=len(pairs) & 1))
    got = check(pairs, 'lengths')
    assert got[0]['cs'] == ':1' and got[0]['md'] == '1' and got[0]['eqx'] == [op(1, 7)]
    p64 = [g for p, g in zip(pairs, got) if p.cigar == [op(64, M)]]
    assert p64[0]['cs'] == ':64' and p64[0]['md'] == '64'


def test_digit_boundaries(lib):
    rng = np.random.default_rng(2)
    pairs = [from_cigar(rng, [op(n + 1, M)], [n], rev=k & 1) for k, n in enumerate((9, 10, 99, 100, 999, 1000, 9999, 10000))]
    # a run of 10000 matching columns interrupted by insertions only: one MD number, several cs runs
    pairs.append(from_cigar(rng, [op(2500, M), op(1, I), op(2500, M), op(2, I), op(2500, M), op(1, I), op(2500, M)]))
    got = check(pairs, 'digits')
    for n, g in zip((9, 10, 99, 100, 999, 1000, 9999, 10000), got):
        assert g['cs'].startswith(':%d*' % n) and g['md'].startswith('%d' % n) and g['md'].endswith('0'), (n, g['cs'], g['md'])
    assert got[-1]['md'] == '10000' and got[-1]['cs'].count(':2500') == 4


def test_adjacent_events(lib):
    rng = np.random.default_rng(3)
    pairs = [
        from_cigar(rng, [op(5, M), op(2, D), op(5, M)], [4, 7]),            # mismatch directly before and after a deletion
        from_cigar(rng, [op(70, M), op(3, D), op(70, M)], [69, 73], rev=1),
        from_cigar(rng, [op(4, M), op(2, D), op(3, I), op(4, M)]),          # deletion and insertion adjacent, both orders
        from_cigar(rng, [op(4, M), op(3, I), op(2, D), op(4, M)], rev=1),
        from_cigar(rng, [op(2, I), op(10, M), op(3, D)]),                   # starting / ending with I / D
        from_cigar(rng, [op(2, D), op(10, M), op(3, I)], [2, 11]),
        from_cigar(rng, [op(3, D), op(2, D), op(4, M)]),                    # (two deletion ops in a row: each has its own ^)
        from_cigar(rng, [op(1, M), op(1, I)] * 3000, rev=1),                # many ops, few columns
        from_cigar(rng, [op(1, M), op(1, D)] * 3000, range(0, 6000, 14)),
        from_cigar(rng, [op(7, I)]),                                        # a single op
        from_cigar(rng, [op(7, D)]),
        from_cigar(rng, [op(1, M)], [0]),
        Pair([], [], [], ql=5, tl=3, tr=4, rng=rng),                         # n_cigar = 0
        Pair([], [], [], rev=1, rng=rng),
    ]
    got = check(pairs, 'adjacent')
    import re
    assert re.match(r'^4[ACGT]0\^[ACGT]{2}0[ACGT]4$', got[0]['md']), got[0]['md']      # 0 between ^.. and the mismatch after it
    assert re.match(r'^0\^[ACGT]{3}0\^[ACGT]{2}4$', got[6]['md']), got[6]['md']
    assert got[-1] == dict(cs='', md='', eqx=[]) and got[-2] == dict(cs='', md='', eqx=[])
    assert got[9]['md'] == '0' and got[9]['eqx'] == [op(7, I)] and got[10]['cs'].startswith('-') and got[11]['md'].startswith('0')


def test_ambiguous_codes(lib):
    rng = np.random.default_rng(4)
    pairs = []
    for rev in (0, 1):
        n = 200
        t = rng.integers(0, 4, n).astype(np.uint8)
        q = t.copy()
        t[10] = q[10] = 4            # N against N: a match
        t[20] = 4                    # N (target) against a base
        q[30] = 4                    # a base against N (read)
        t[50:140] = 4                # runs of N crossing the chunk boundaries at 64 and 128
        q[60:130] = 4
        pairs.append(Pair([op(n, M)], q, t, rev=rev, ql=3, qr=2, tl=5, tr=7, rng=rng))
        # N inside an insertion and a deletion, N runs at both ends
        t2 = rng.integers(0, 4, 150).astype(np.uint8)
        t2[:3] = 4
        t2[70:75] = 4
        t2[-2:] = 4
        q2 = np.concatenate([t2[:60], [4, 0, 4], t2[60:70], t2[75:]]).astype(np.uint8)
        pairs.append(Pair([op(60, M), op(3, I), op(10, M), op(5, D), op(75, M)], q2, t2, rev=rev, ql=1, tl=14, rng=rng))
    got = check(pairs, 'N')
    assert '*na' in got[0]['cs'] or '*nc' in got[0]['cs'] or '*ng' in got[0]['cs'] or '*nt' in got[0]['cs']
    assert 'n' in got[1]['cs'] and '^NNNNN' in got[1]['md'] and got[1]['md'].endswith('75')


def test_every_word_offset_on_both_strands(lib):
    """the first aligned base at every offset of a 4-byte read word and of a 16-base target word, on each strand by itself; the
    alignment ends at the very last base of the read (in the alignment's orientation) and of the target"""
    rng = np.random.default_rng(5)
    pairs, cum_q, cum_t = [], 0, 0     # reads and targets are concatenated in the call: what precedes a pair moves its words
    for rev in (0, 1):
        for a in range(16):
            ln = 61 + 3 * a
            tl = (a - cum_t) % 16                      # the first aligned target base at offset a of its 2-bit word
            if rev:
                # the alignment's first base is the LAST aligned base of the read, its last one is the read's base 0 (no left
                # flank): the length of the last M op puts the first one at offset a % 4 of its word
                last = 40 + (a % 4 - (cum_q + ln + 2 + 9 + 40 - 1)) % 4
                kw = dict(ql=0, qr=a % 3)
            else:
                last = 40 + a % 5
                kw = dict(ql=(a % 4 - cum_q) % 4, qr=0)
            p = from_cigar(rng, [op(ln, M), op(2, I), op(9, M), op(3, D), op(last, M)], [0, ln - 1, ln + 5], rev=rev, tl=tl, tr=0, **kw)
            p.off_q = (cum_q + (p.qe - 1 if rev else p.qs)) % 4
            p.off_t = (cum_t + p.ts) % 16
            assert (p.off_q, p.off_t) == (a % 4, a) and p.ts + len(p.t) == len(p.target) and (p.qs == 0 if rev else p.qe == len(p.read))
            cum_q += len(p.read)
            cum_t += len(p.target)
            pairs.append(p)
    got = check(pairs, 'offsets')
    for rev in (0, 1):
        assert {p.off_q for p in pairs if p.rev == rev} == set(range(4)), rev
        assert {p.off_t for p in pairs if p.rev == rev} == set(range(16)), rev
        assert {(p.off_q, p.off_t) for p in pairs if p.rev == rev} == {(a % 4, a) for a in range(16)}
    assert all(g['md'].startswith('0') for g in got)


def test_alignment_beyond_the_lds_classes(lib):
    rng = np.random.default_rng(6)
    p = random_pair(rng, 70000, 0.12, ql=2, qr=5, tl=9, tr=3)
    assert len(p.cigar) > 4096 and sum(c >> 4 for c in p.cigar) == 70000
    pr = random_pair(rng, 70000, 0.12, rev=1, ql=1, tl=30)
    check([p, pr], '70k columns')


def test_random_batch(lib):
    rng = np.random.default_rng(7)
    pairs = []
    for k in range(300):
        length = int(rng.integers(1, 3001)) if k % 10 else int(rng.integers(1, 70))
        err = float(rng.choice([0.0, 0.02, 0.1, 0.2, 0.3]))
        pairs.append(random_pair(rng, length, err, rev=int(rng.integers(0, 2)), ql=int(rng.integers(0, 9)), qr=int(rng.integers(0, 9)),
                                 tl=int(rng.integers(0, 40)), tr=int(rng.integers(0, 40))))
    n_ops = [len(p.cigar) for p in pairs]
    assert min(n_ops) == 1 and any(512 < n <= 4096 for n in n_ops) and any(n <= 512 for n in n_ops), (min(n_ops), max(n_ops))
    check(pairs, 'random')


def test_argument_errors(lib):
    from megapath_nano_amd import _ffi
    rng = np.random.default_rng(8)
    good = from_cigar(rng, [op(30, M), op(2, I), op(30, M)], [7])
    for bad_cigar in ([op(30, M), op(2, I), op(29, M)],      # does not consume its read interval
                      [op(30, M), op(2, I), op(31, M)],
                      [op(62, 4)],                           # a soft clip: not M / I / D
                      [op(30, M), op(2, I), op(30, M), op(50, D)]):   # leaves the target
        bad = from_cigar(rng, [op(30, M), op(2, I), op(30, M)])
        bad.cigar = bad_cigar
        with pytest.raises(_ffi.MpnError, match=r'rc=-1'):
            run([good, bad], CS | MD | EQX)
    with pytest.raises(_ffi.MpnError, match=r'rc=-3'):
        run([good, good], CS | MD | EQX, caps=(3, 1000, 1000))
    with pytest.raises(_ffi.MpnError, match=r'rc=-3'):
        run([good], CS | MD | EQX, caps=(1000, 1000, 1))
    assert run([good], CS | MD | EQX)[0]['cs'] == write_tags(good.cigar, good.q, good.t)['cs']
