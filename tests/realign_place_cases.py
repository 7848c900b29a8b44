"""Small constructed windows for the realigner's placement stage (realigner.place_batch), in named families.  Every case is
(family, name, window); tests/test_realign_place_ref.py asserts that each reaches what it is named for, and
tests/test_realign_place_gpu.py compares the stage with tests/realign_place_ref.py on all of them."""
import functools

import numpy as np

import realign_place_ref as ref

BASES = 'ACGT'
OFF = 1 << 20          # a ref_prefix no position reaches: the coverage test never fires
UNIT = 'ACCGTAG'       # period 7 and no shorter one


def rand_seq(rng, n):
    return ''.join(BASES[i] for i in rng.integers(0, 4, n))


def sub(s, i, to=None):
    """s with the base at i substituted (by the next base, or by `to`)"""
    c = to if to is not None else BASES[(BASES.index(s[i].upper()) + 1) % 4]
    assert c != s[i]
    return s[:i] + c + s[i + 1:]


def window(seqs, haplotypes, reference=None, ref_prefix=OFF, ref_suffix=0):
    if reference is None:   # close to the first haplotype and never equal to one: no haplotype is the reference
        reference = sub(haplotypes[0], len(haplotypes[0]) // 2) if haplotypes else 'ACGT' * 16
        assert reference not in haplotypes
    return dict(seqs=list(seqs), positions=[100 + r for r in range(len(seqs))], cigars=['%dM' % len(s) for s in seqs],
                reference=reference, haplotypes=list(haplotypes), ref_start=1000, ref_prefix=ref_prefix, ref_suffix=ref_suffix)


# ---- lengths -------------------------------------------------------------------------------------------------------------
LENGTHS_L = (0, 1, 31, 32, 33, 34, 64, 96, 97, 250)
LENGTHS_HL = (32, 33, 64, 96, 128, 160)
# HL + L - 63 diagonals hold a k-mer: 63, 64, 65 and 127, 128, 129 of them (1 is HL == L == 32, in the product)
LENGTHS_EXTRA = {64: (62, 63), 96: (94, 95)}


def _lengths():
    out = []
    for HL in LENGTHS_HL:
        rng = np.random.default_rng(300 + HL)
        hap = rand_seq(rng, HL)
        seqs = []
        for L in LENGTHS_L + LENGTHS_EXTRA.get(HL, ()):
            if L <= HL:
                seqs.append(hap[HL - L:])                                    # ends with the haplotype
                seqs.append(sub(hap[:L], L - 1) if L >= 1 else hap[:L])      # starts with it, its last base a mismatch
            else:                                                            # longer than the haplotype: k-mers, no placement
                seqs.append(rand_seq(rng, min(3, L - HL)) + hap + rand_seq(rng, L - HL - min(3, L - HL)))
                seqs.append(hap + rand_seq(rng, L - HL))
        out.append(('lengths', 'hl%d' % HL, window(seqs, [hap])))
    return out


# ---- clamp ---------------------------------------------------------------------------------------------------------------
def _repeat_pair(rng, read_len, read_subs, hap_subs, lead=0):
    """haplotype: `lead` random bases, 120 of the period-7 repeat, a random tail; read: its first read_len bases; then the
    substitutions"""
    hap = rand_seq(rng, lead) + (UNIT * 18)[:120] + rand_seq(rng, 40)
    read = hap[:read_len]
    for i in hap_subs:
        hap = sub(hap, i)
    for i in read_subs:
        read = sub(read, i)
    return read, hap


def _far_pair(rng):
    """start 0 with no mismatch and no 32-mer on diagonal 0 (an N every < 32 bases, in one of the two), and read[80:112] ==
    haplotype[10:42] including an N: the only k-mer match lies on diagonal -70"""
    b = list(rand_seq(rng, 160))
    b[80:112] = b[10:42]
    hap, read = b[:], b[:120]
    hap[25] = 'N'
    read[95] = 'N'
    hap[50] = 'N'
    hap[72] = 'N'
    return ''.join(read), ''.join(hap)


def _clamp():
    rng = np.random.default_rng(41)
    pairs = [
        ('only_clamp', _repeat_pair(rng, 70, [20], [46])),         # the issue's case: t = 0 through read offset 21
        ('same_t', _repeat_pair(rng, 70, [45], [5])),              # diagonal 0 and diagonal -7 both first match at t = 6
        ('own_earlier', _repeat_pair(rng, 70, [], [], lead=10)),   # diagonal 0 at t = 0, diagonal -7 at t = 10
        ('own_later', _repeat_pair(rng, 70, [20], [60])),          # diagonal 0 at t = 21, diagonal -21 at t = 0
        ('three_mm', _repeat_pair(rng, 70, [20, 65], [46])),       # start 0 with 3 mismatches
        ('far', _far_pair(rng)),                                   # the matching diagonal is 70 away from 0
        ('two_negative', _repeat_pair(rng, 60, [20], [46])),       # diagonals -7, -14, -21, -28 at t = 14, 7, 0, 0
    ]
    return [('clamp', name, window([read], [hap])) for name, (read, hap) in pairs]


# ---- letters -------------------------------------------------------------------------------------------------------------
def _letters():
    rng = np.random.default_rng(52)
    hap = rand_seq(rng, 120)
    hn = sub(hap, 30, 'N')
    hl = hap[:70] + hap[70].lower() + hap[71:]
    read = hap[10:90]
    cases = [
        ('n_both', [hn[10:60]], [hn]),                                # the N inside every matching 32-mer
        ('n_read', [sub(hap[10:80], 5, 'N')], [hap]),
        ('n_hap', [hap[10:80]], [hn]),
        ('lower_read', [read[:40] + read[40].lower() + read[41:], read.lower()], [hap]),
        ('lower_both', [hl[20:100], hap[20:100]], [hl]),
        ('mm2', [sub(sub(read, 3), 40)], [hap]),
        ('mm3', [sub(sub(sub(read, 3), 40), 44)], [hap]),
        ('first_last', [sub(sub(read, 0), len(read) - 1)], [hap]),
        ('n_and_mm', [sub(sub(sub(read, 2, 'N'), 3), 40)], [hn]),     # 2 mismatches and an N on each side
    ]
    return [('letters', name, window(seqs, haps)) for name, seqs, haps in cases]


# ---- ties ----------------------------------------------------------------------------------------------------------------
def _ties():
    rng = np.random.default_rng(63)
    tandem = rand_seq(rng, 20) + UNIT * 12 + rand_seq(rng, 20)
    rep = (UNIT * 8)
    hap = rand_seq(rng, 110)
    cases = [
        ('tandem', [rep[:40], rep[3:45], sub(rep[:47], 4), tandem[10:60]], [tandem, sub(tandem, 50)]),
        ('identical', [hap[20:70]] * 3 + [rep[:40]] * 2, [hap, tandem]),
        ('meet', [hap[10:60], hap[0:50], hap[5:45]], [hap]),          # at t = 10 .. 13 the k-mer is in all three reads
    ]
    return [('ties', name, window(seqs, haps)) for name, seqs, haps in cases]


# ---- coverage ------------------------------------------------------------------------------------------------------------
def _decoy(rng, hap, x, flank=5, tail=None):
    """a read that holds the haplotype's 32-mer at x and cannot be placed: random flanks (more than 2 mismatches), or with
    `tail` a tail that runs over the haplotype's end"""
    return rand_seq(rng, flank) + hap[x:x + 32] + rand_seq(rng, flank if tail is None else tail)


def _coverage():
    rng = np.random.default_rng(74)
    hap = rand_seq(rng, 160)
    head = hap[:40]                       # placed at 0: covers its own k-mer positions, gives the haplotype a score
    P, S = 60, 40
    cases = [
        ('below_prefix', [head, _decoy(rng, hap, P - 1)], hap, None, P, S),
        ('at_prefix', [head, _decoy(rng, hap, P)], hap, None, P, S),
        ('below_suffix', [head, _decoy(rng, hap, 160 - S - 1)], hap, None, P, S),
        ('at_suffix', [head, _decoy(rng, hap, 160 - S)], hap, None, P, S),
        ('suffix_over_hl', [head, _decoy(rng, hap, 100)], hap, None, P, 500),
        ('prefix_zero', [head, _decoy(rng, hap, 50)], hap, None, 0, S),
        ('prefix_zero_at_0', [_decoy(rng, hap, 0), hap[100:160]], hap, None, 0, S),
        ('no_kmer', [head, hap[100:160]], hap, None, 0, 0),
        ('decoy_no_fit', [head, _decoy(rng, hap, 110, tail=60)], hap, None, P, 10),
        ('late', [head, _decoy(rng, hap, 60), sub(hap[50:130], 30)], hap, None, 50, 10),
        ('in_time', [head, _decoy(rng, hap, 60), hap[50:130]], hap, None, 50, 10),
        ('is_reference', [head, _decoy(rng, hap, 100)], hap, hap, P, S),
        ('zero_score', [rand_seq(rng, 50), _decoy(rng, hap, 20)], hap, None, P, S),
    ]
    return [('coverage', name, window(seqs, [h], reference=r, ref_prefix=p, ref_suffix=s)) for name, seqs, h, r, p, s in cases]


# ---- shapes --------------------------------------------------------------------------------------------------------------
def _shapes():
    rng = np.random.default_rng(85)
    haps = [rand_seq(rng, 90 + 7 * k) for k in range(3)]
    reads = [haps[k % 3][5 + k:50 + 2 * k] for k in range(5)]
    cases = [
        ('no_reads', [], haps[:2]),
        ('no_haplotypes', reads[:3], []),
        ('short_reads', [haps[0][:32], haps[0][3:20], haps[1][40:71]], haps[:2]),
        ('pairs1', reads[:1], haps[:1]),
        ('pairs3', reads[:3], haps[:1]),
        ('pairs4', reads[:2], haps[:2]),
        ('pairs5', reads[:5], haps[:1]),
        ('pairs9', reads[:3], haps[:3]),
    ]
    return [('shapes', name, window(seqs, hs)) for name, seqs, hs in cases]


FAMILIES = ('lengths', 'clamp', 'letters', 'ties', 'coverage', 'shapes')


@functools.lru_cache(maxsize=None)
def make_cases():
    cases = _lengths() + _clamp() + _letters() + _ties() + _coverage() + _shapes()
    assert {f for f, _, _ in cases} == set(FAMILIES) and len({(f, n) for f, n, _ in cases}) == len(cases)
    return tuple(cases)


def case(family, name):
    return next(w for f, n, w in make_cases() if (f, n) == (family, name))


# ---- the natural overflow of the placement list ---------------------------------------------------------------------------
ALL_A_HITS = 40 * (1700 - 33 + 1)     # 66 720, above the 65 536 the list starts with


@functools.lru_cache(maxsize=None)
def all_a_window():
    """one all-A haplotype of 1700 bases and 40 reads of 33 A: every read fits every start"""
    w = window(['A' * 33] * 40, ['A' * 1700])
    return w


# ---- the restatement's results, computed once and shared -------------------------------------------------------------------
_placed = {}


def placed(w):
    """realign_place_ref.place_window(w), computed once per window (callers leave it unchanged)"""
    key = id(w)
    if key not in _placed:
        _placed[key] = (w, ref.place_window(**w))
    return _placed[key][1]
