"""Constructed windows for the de Bruijn graph consensus: the smallest shapes at which a rule of debruijn_graph.cpp (or the table,
the walk and the sort of csrc/dbg_core.h) can go wrong, shared by the restatement's, the host build's and the kernel's tests.

A case is a dict: name, ref, reads, bad (one set of positions per read) and, where the answer was derived by hand from the
reference's source, `n` (haplotypes) and `k`.  host_run() runs cases through scripts/dbg_host_check.cpp."""
import os
import random
import struct
import subprocess

import dbg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rnd(n, seed):
    r = random.Random(seed)
    return ''.join(r.choice('ACGT') for _ in range(n))


def snp(s, pos):
    return s[:pos] + 'ACGT'[('ACGT'.index(s[pos]) + 1) % 4] + s[pos + 1:]


def case(name, ref, reads, bad=None, **want):
    bad = [set() for _ in reads] if bad is None else [set(b) for b in bad]
    assert len(bad) == len(reads)
    return dict(name=name, ref=ref, reads=list(reads), bad=bad, **want)


R60 = rnd(60, 1)          # every 10-mer distinct (test_dbg_ref checks it): k = 10 unless a read forces more
S30 = snp(R60, 30)
R150 = rnd(150, 22)       # for the windows whose k is raised: long enough that a SNP at 75 still has both flanks at k = 40
S75 = snp(R150, 75)


def bounds():
    u30, u101 = rnd(30, 2), rnd(101, 3)
    return [case('ref_10', rnd(10, 4), [], n=0, k=0),                  # max_k = 9 < 10
            case('ref_11', rnd(11, 5), [], n=1, k=10),
            case('ref_12', rnd(12, 6), [], n=1, k=10),
            case('homopolymer_50', 'A' * 50, [], n=0, k=0),
            case('repeat_30mer', u30 + u30, [], n=1, k=31),            # 30-mers repeat, 31-mers do not
            case('repeat_101mer', u101 + u101, [], n=0, k=0)]           # the 101-mer at 0 and at 101: no k up to max_k = 101


def reads():
    k = 10
    at = 25                                                             # reads cut so that the SNP at 30 is inside
    return [case('no_reads', R60, [], n=1, k=10),
            case('one_empty_read', R60, [''], n=1, k=10),
            case('shorter_than_k', R60, [S30[at:at + k - 3]] * 2, n=1, k=10),
            case('exactly_k', R60, [S30[at:at + k]] * 2, n=1, k=10),      # adds nothing
            case('k_plus_1', R60, [S30[at:at + k + 1]] * 2, n=1, k=10),   # one edge that goes nowhere
            case('snp_read_12', R60, [S30[24:36]] * 2, n=1, k=10),        # cannot close the bubble
            case('snp_read_21', R60, [S30[20:41]] * 2, n=2, k=10)]        # 11 edges: ref 10-mer, ten with the SNP, ref 10-mer


def support():
    ins = R60[:30] + 'GAT' + R60[30:]
    dele = R60[:28] + R60[31:]
    n_ref = R60[:15] + 'N' + R60[16:]
    low = S30[:22] + S30[22].lower() + S30[23:]
    low_far = S30[:5] + S30[5].lower() + S30[6:]
    with_n = S30[:35] + 'N' + S30[36:]
    out = [case('snp_one_read', R60, [S30], n=1, k=10),
           case('snp_two_reads', R60, [S30, S30], n=2, k=10),
           case('snp_bad_at_snp', R60, [S30, S30], [{30}, {30}], n=1, k=10),
           case('snp_bad_in_one_read', R60, [S30, S30], [{30}, set()], n=1, k=10),
           case('reference_reads_only', R60, [R60[3:40]] * 3, n=1, k=10)]
    # an edge needs k + 1 = 11 good bases: the bubble's first edge is bases 20 .. 30, its last 30 .. 40
    for d, n in ((-11, 2), (-10, 1), (0, 1), (10, 1), (11, 2)):
        out.append(case('snp_bad_at_%+d' % d, R60, [S30, S30], [{30 + d}, {30 + d}], n=n, k=10))
    out += [case('lower_case_near', R60, [low, low], n=1, k=10),
            case('lower_case_far', R60, [low_far, low_far], n=2, k=10),
            case('n_in_read', R60, [with_n, with_n], n=1, k=10),
            case('n_in_reference', n_ref, [snp(n_ref, 40)[20:]] * 2, n=2, k=10),
            case('n_in_reference_and_reads', n_ref, [snp(n_ref, 40)] * 2, n=2, k=10),
            case('insertion', R60, [ins, ins], n=2, k=10),
            case('deletion', R60, [dele, dele], n=2, k=10),
            case('insertion_deletion_snp', R60, [ins, ins, dele, dele, S30, S30], k=10)]
    return out


def dangling():
    past = rnd(17, 7) + S30 + rnd(23, 8)
    branch = R60[10:30] + rnd(25, 9)
    return [case('past_both_ends', R60, [past, past], n=2, k=10),
            case('branch_never_returns', R60, [branch, branch], n=1, k=10),
            case('branch_and_snp', R60, [branch, branch, S30, S30], n=2, k=10)]


def cycles():
    # reference x t y t z with a repeated 10-mer t (so min_k = 11), then a 12-mer u, then a tail that begins with u's first base:
    # the reads carry u four times, 49 bases of period 12 with that base, so k-mers repeat while k + 12 <= 49 and k = 38 is the first
    t, u = rnd(10, 10), rnd(12, 11)
    x, y, z = rnd(20, 12), rnd(7, 13), rnd(30, 14)
    y = y[:-1] + snp(y, 6)[6] if y[-1] == x[-1] else y          # the two copies of t differ in the base before and behind,
    z = snp(z, 0) if z[0] == y[0] else z                          # so that every 11-mer of the reference is distinct
    left = x + t + y + t + z
    tail = rnd(60, 15)
    tail = u[0] + tail[1:] if tail[0] != u[0] else tail
    tandem_ref, tandem_read = left + u + tail, left + u * 4 + tail
    junk40, junk120 = rnd(20, 16) + 'A' * 40 + rnd(20, 17), rnd(5, 18) + 'A' * 120 + rnd(5, 19)
    return [case('tandem_12mer', tandem_ref, [tandem_read, tandem_read], n=2, k=38),
            case('junk_a40', R150, [S75, S75, junk40], n=2, k=40),                       # self-loops while k + 1 <= 40
            case('junk_a40_one_bad', R150, [S75, S75, junk40], [set(), set(), {40}], n=2, k=20),      # runs of 20 and 19 A
            case('junk_a40_bad_every_8', R150, [S75, S75, junk40], [set(), set(), set(range(20, 60, 8))], n=2, k=10),
            case('junk_a120', R150, [S75, S75, junk120], n=0, k=0)]


def bubbles(n):
    ref = rnd(30 + 15 * n, 20)
    alt = ref
    for b in range(n):
        alt = snp(alt, 15 + 15 * b)
    return ref, alt


def cap():
    out = []
    for n, want in ((8, 256), (9, 0)):
        ref, alt = bubbles(n)
        out.append(case('bubbles_%d' % n, ref, [alt, alt], n=want, k=10))
    return out


def noisy_window(seed, ref_len, n_reads, read_len, err, variants=0):
    r = random.Random(seed)
    ref = ''.join(r.choice('ACGT') for _ in range(ref_len))
    alt = ref
    for v in range(variants):
        alt = snp(alt, (v + 1) * ref_len // (variants + 1))
    out, bad = [], []
    for i in range(n_reads):
        n = read_len if isinstance(read_len, int) else r.randint(*read_len)
        n = min(n, ref_len)
        s = r.randint(0, ref_len - n)
        src = alt if i % 2 else ref
        out.append(''.join(r.choice('ACGT') if r.random() < err else c for c in src[s:s + n]))
        bad.append({r.randrange(n) for _ in range(r.randint(0, 3))})
    return ref, out, bad


def table():
    ref, rd, bad = noisy_window(21, 400, 300, 250, 0.01, variants=2)
    ref2, rd2, bad2 = noisy_window(23, 400, 60, 250, 0.005, variants=2)
    # at this depth the errors that two reads share make more than 256 paths: the first window ends at the cap, the second does not
    return [case('noisy_300x250', ref, rd, bad, n=0), case('noisy_60x250', ref2, rd2, bad2)]


FAMILIES = dict(bounds=bounds, reads=reads, support=support, dangling=dangling, cycles=cycles, cap=cap, table=table)


def all_cases():
    return [c for f in FAMILIES.values() for c in f()]


def small_cases():
    return [c for name, f in FAMILIES.items() if name != 'table' for c in f()]


_want = {}


def expected(c):
    """(haplotypes, k) of the restatement, computed once per case"""
    if c['name'] not in _want:
        _want[c['name']] = dbg_ref.get_consensus(c['ref'], c['reads'], c['bad'])
    return _want[c['name']]


def random_small_window(r):
    """A window of a few dozen bases over a small alphabet of events: repeats, variants, bad bases, odd letters, short reads"""
    n = r.randint(9, 40)
    ref = ''.join(r.choice('ACGT' if r.random() < 0.9 else 'AC') for _ in range(n))
    if r.random() < 0.1:
        ref = ref[:r.randrange(n)] + r.choice('NRacgt') + ref[r.randrange(n):]
    rd, bad = [], []
    for _ in range(r.randint(0, 6)):
        a = r.randrange(len(ref))
        s = ref[a:a + r.randint(0, len(ref))]
        for _ in range(r.randint(0, 2)):
            if s:
                p = r.randrange(len(s))
                s = r.choice([s[:p] + r.choice('ACGTNa') + s[p + 1:], s[:p] + s[p + 1:], s[:p] + r.choice('ACGT') * r.randint(1, 12) + s[p:]])
        copies = r.randint(1, 2)
        rd += [s] * copies
        bad += [{r.randrange(len(s) + 2) for _ in range(r.choice((0, 0, 1, 2)))} for _ in range(copies)]
    return ref, rd, bad


# ---- the host build --------------------------------------------------------------------------
OK, NO_K, PATH_CAP, TABLE_FULL, HAP_FULL = range(5)
OVER_THE_CAP = ('bubbles_9', 'noisy_300x250')


def expected_status(c):
    return NO_K if expected(c)[1] == 0 else PATH_CAP if c['name'] in OVER_THE_CAP else OK


def build_host_check(out_dir, optimised=False):
    exe = os.path.join(str(out_dir), 'dbg_host_check')
    base = ['g++', '-std=c++17', '-Wall', '-Werror', '-o', exe, os.path.join(ROOT, 'scripts', 'dbg_host_check.cpp')]
    if optimised or subprocess.run(base + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']).returncode != 0:
        subprocess.run(base + ['-O2'], check=True)
    return exe


def pack(windows, slots=0, grow=1):
    """windows: (ref, reads, bad sets) -> the bytes of a case file of scripts/dbg_host_check.cpp"""
    out = [struct.pack('<I', len(windows))]
    for ref, rd, bad in windows:
        out.append(struct.pack('<III', slots, grow, len(ref)) + ref.encode() + struct.pack('<I', len(rd)))
        for s, b in zip(rd, bad):
            out.append(struct.pack('<I', len(s)) + s.encode() + bytes(1 if i in b else 0 for i in range(len(s))))
    return b''.join(out)


def host_run(exe, tmp, windows, slots=0, grow=1):
    """-> [(status, k, haplotypes, times redone)]"""
    src, dst = os.path.join(str(tmp), 'dbg_cases.bin'), os.path.join(str(tmp), 'dbg_results.bin')
    with open(src, 'wb') as f:
        f.write(pack(windows, slots, grow))
    subprocess.run([exe, 'run', src, dst], check=True, timeout=600)
    blob, p, out = open(dst, 'rb').read(), 0, []
    for _ in windows:
        status, k, n, redone = struct.unpack_from('<4i', blob, p)
        p += 16
        haps = []
        for _ in range(n):
            size, = struct.unpack_from('<I', blob, p)
            haps.append(blob[p + 4:p + 4 + size].decode())
            p += 4 + size
        out.append((status, k, haps, redone))
    assert p == len(blob)
    return out
