"""A plain restatement of what megapath_nano_amd/clair_call.py computes: output_with / output_from of Clair's clair/call_var.py and
its pysam look-ups, in Python and numpy float32 scalars.

Two forms of the pile-up column of a site:
  * literal_sequences: a sequential restatement of htslib's pile-up machine (the list of nodes, cnt, max_pos, the drop rule of
    bam_plp_push, bam_plp64_next, resolve_cigar2 with its per-read state) and of the spelling of samtools' pileup_seq;
  * closed_sequences: the closed form the product uses (the first 250 taken reads, and the first of every start position; the
    operation that covers the column found by a walk), with the same spelling.
tests/test_clair_call_ref.py checks that the two agree on random read sets.

A read is (flag, pos0, [(op, n), ..] with op in 'MIDNSHP=X', seq).  Not modelled: overlap detection of pairs, BAQ, pysam's own
version differences.

promotion: 'legacy' is NumPy 1.x (`1.0 - p` and `count + 0.0` are float64: what the reference's environment computes and what the
product implements); 'nep50' is NumPy 2.x (both stay float32: what the goldens were recorded with)."""
import math

import numpy as np

FLANK = 16
MAX_DEPTH = 250
MAX_LEN = 50
FILTER_FLAG = 2316
F32 = np.float32
GT21 = ['AA', 'AC', 'AG', 'AT', 'CC', 'CG', 'CT', 'GG', 'GT', 'TT', 'DelDel', 'ADel', 'CDel', 'GDel', 'TDel', 'InsIns', 'AIns', 'CIns', 'GIns', 'TIns', 'InsDel']
HOMO, HETERO = [0, 4, 7, 9], [1, 2, 3, 5, 6, 8]
GENOTYPES = ['0/0', '1/1', '0/1', '1/2']
BASE2NUM = dict(zip('ACGTURYSWKMBDHVN', (0, 1, 2, 3, 3, 0, 1, 1, 0, 2, 0, 1, 0, 0, 0, 0)))
BASE2ACGT = dict(zip('ACGTURYSWKMBDHVN', 'ACGTTACCAGACAAAA'))
ON_REF = 'MDN=X'


def parse_cigar(text):
    out, n = [], ''
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((ch, int(n)))
            n = ''
    return out


def read_of(sam_line):
    """a SAM line -> (flag, pos0, cigar, seq)"""
    f = sam_line.split('\t')
    return int(f[1]), int(f[3]) - 1, parse_cigar(f[5]) if f[5] != '*' else [], f[9]


def rlen(cigar):
    return sum(n for op, n in cigar if op in ON_REF)


def overlapping(reads, position):
    """the reads a fetch of the 0-based base `position` gives a pile-up with flag_filter 2316, in file order"""
    return [r for r in reads if not (r[0] & FILTER_FLAG) and r[1] < position + 1 and r[1] + max(rlen(r[2]), 1) > position]


# ---- the spelling ----------------------------------------------------------------------------------------------------------------
def peek(cigar, k, x, pos):
    """resolve_cigar2's look at the next operation -> indel"""
    op, n = cigar[k]
    indel = 0
    if x + n - 1 == pos and k + 1 < len(cigar):
        op2, l2 = cigar[k + 1]
        if op2 == 'D':
            indel = -l2
        elif op2 == 'I':
            indel = l2
        elif op2 == 'P' and k + 2 < len(cigar):
            l3 = 0
            for o, l in cigar[k + 2:]:
                if o == 'I':
                    l3 += l
                elif o in ON_REF:
                    break
            if l3 > 0:
                indel = l3
    return indel


def spell(read, k, x, y, pos):
    """pileup_seq without reference and without the marks of ends, for the read whose operation k (from reference x, query y) covers pos"""
    flag, _, cigar, seq = read
    rev = bool(flag & 16)
    op, n = cigar[k]
    indel = peek(cigar, k, x, pos)
    is_del = op in 'DN'
    qpos = y if is_del else y + (pos - x)
    if not is_del:
        c = seq[qpos] if qpos < len(seq) and seq != '*' else 'N'
        c = (',' if rev else '.') if c == '=' else (c.lower() if rev else c.upper())
    else:
        c = ('<' if rev else '>') if op == 'N' else '*'
    out = c
    del_len = -indel
    if indel > 0:
        del_len, ins, j = 0, '', 1
        for o, l in cigar[k + 1:]:
            if o == 'P':
                ins += '*' * l
            elif o == 'I':
                for _ in range(l):
                    q = qpos + j - (1 if is_del else 0)
                    if seq == '*' or q >= len(seq):
                        raise IndexError('an inserted base past the bases of the read')
                    ins += seq[q]
                    j += 1
            else:
                if o == 'D':
                    del_len = l
                break
        out += '+%d' % len(ins) + ''.join(ch if ch == '*' else (ch.lower() if rev else ch.upper()) for ch in ins)
    if del_len > 0:
        out += '-%d' % del_len + ('n' if rev else 'N') * del_len
    return out


def covering(read, pos):
    """the operation of the read that covers the 0-based reference position pos -> (k, x, y) or None"""
    x, y = read[1], 0
    for k, (op, n) in enumerate(read[2]):
        if op in ON_REF:
            if x <= pos < x + n:
                return k, x, y
            x += n
        if op in 'MIS=X':
            y += n
    return None


def closed_members(reads, position):
    """the reads of the column of the 0-based position - 1, by the closed form"""
    col, out, last = position - 1, [], None
    for i, r in enumerate(overlapping(reads, position)):
        first = last is None or r[1] != last
        last = r[1]
        if (i < MAX_DEPTH or first) and r[1] <= col < r[1] + rlen(r[2]):
            out.append(r)
    return out


def closed_sequences(reads, position):
    col = position - 1
    return [spell(r, *covering(r, col), col) for r in closed_members(reads, position)]


class _Node:
    def __init__(self, read):
        self.read, self.beg, self.end = read, read[1], read[1] + rlen(read[2])
        self.k, self.x, self.y = -1, 0, 0


def _resolve(node, pos):
    """resolve_cigar2: moves the node's state to pos -> (k, x, y)"""
    cigar = node.read[2]
    if node.k == -1:
        if len(cigar) == 1:
            if cigar[0][0] in 'M=X':
                node.k, node.x, node.y = 0, node.beg, 0
        else:
            node.x, node.y, k = node.beg, 0, 0
            while k < len(cigar):
                op, n = cigar[k]
                if op in ON_REF:
                    break
                if op in 'IS':
                    node.y += n
                k += 1
            assert k < len(cigar)
            node.k = k
    else:
        n = cigar[node.k][1]
        if pos - node.x >= n:
            if cigar[node.k][0] in 'M=X':
                node.y += n
            node.x += n
            k = node.k + 1
            while k < len(cigar):
                op, l = cigar[k]
                if op in ON_REF:
                    break
                if op in 'IS':
                    node.y += l
                k += 1
            assert k < len(cigar)
            node.k = k
    return node.k, node.x, node.y


class Pileup:
    """bam_plp_t for one contig: push, next and the auto loop over an iterator of reads"""

    def __init__(self, reads, maxcnt=MAX_DEPTH):
        self.it, self.maxcnt = iter(reads), maxcnt
        self.nodes, self.cnt, self.pos, self.max_pos, self.is_eof, self.tail_beg = [], 1, 0, -1, False, 0
        self.pushed = []

    def push(self, read):
        if read is None:
            self.is_eof = True
            return
        if self.pos == read[1] and self.cnt > self.maxcnt:
            return
        node = _Node(read)
        self.tail_beg = node.beg
        assert node.beg >= self.max_pos, 'the input is not sorted'
        self.max_pos = node.beg
        if node.end > self.pos:
            self.nodes.append(node)
            self.pushed.append(read)
            self.cnt += 1
            self.tail_beg = 0

    def next(self):
        if self.is_eof and not self.nodes:
            return None
        while self.is_eof or self.max_pos > self.pos:
            column, keep = [], []
            for p in self.nodes:
                if p.end <= self.pos:
                    self.cnt -= 1
                    continue
                keep.append(p)
                if p.beg <= self.pos:
                    column.append((p.read,) + _resolve(p, self.pos))
            self.nodes = keep
            at = self.pos
            head_beg = self.nodes[0].beg if self.nodes else self.tail_beg
            self.pos = head_beg if self.pos < head_beg else self.pos + 1
            if column:
                return at, column
            if self.is_eof and not self.nodes:
                break
        return None

    def auto(self):
        got = self.next()
        if got is not None:
            return got
        if self.is_eof:
            return None
        for read in self.it:
            self.push(read)
            got = self.next()
            if got is not None:
                return got
        self.push(None)
        return self.next()


def literal_column(reads, position):
    """the reads of the column position - 1, with their states, by the machine"""
    plp = Pileup(overlapping(reads, position))
    while True:
        got = plp.auto()
        if got is None:
            return []
        if got[0] == position - 1:
            return got[1]
        if got[0] > position - 1:
            return []


def literal_sequences(reads, position):
    return [spell(read, k, x, y, position - 1) for read, k, x, y in literal_column(reads, position)]


# ---- the look-ups ------------------------------------------------------------------------------------------------------------------
def _number(sequence):
    n, i = 0, 2
    while i < len(sequence) and sequence[i].isdigit():
        n = n * 10 + int(sequence[i])
        i += 1
    return n, sequence[i:]


def insertion_lookup(sequences, lo, hi, ignore=''):
    seen = {}
    for s in sequences:
        if len(s) < 4 or s[1] != '+':
            continue
        n, rest = _number(s)
        rest = rest.upper()
        if lo <= n <= hi and rest != ignore:
            seen[rest] = seen.get(rest, 0) + 1
    return max(seen, key=seen.get) if seen else ''


def deletion_lookup(sequences, fetch, position, lo, hi):
    seen = {}
    for s in sequences:
        if len(s) < 4 or s[1] != '-':
            continue
        n, _ = _number(s)
        key = fetch(position, position + n)
        if lo <= n <= hi:
            seen[key] = seen.get(key, 0) + 1
    return max(seen, key=seen.get) if seen else ''


def events_of(sequences, position, contig_len):
    """what mpn_call_indels lists for the sequences of a column: [(kind, len, count, rank, clip, bases)] in the order of first
    appearance; events longer than 50 are left out.  clip of an insertion: the deletion spelled behind it; its text is None when
    the key is longer than 50 bytes."""
    out, index = [], {}
    for rank, s in enumerate(sequences):
        if len(s) < 4 or s[1] not in '+-':
            continue
        n, rest = _number(s)
        if n < 1 or n > MAX_LEN:
            continue
        key = (0, n, rest.upper()) if s[1] == '+' else (1, n, '')
        if key in index:
            out[index[key]][2] += 1
            continue
        index[key] = len(out)
        if key[0] == 0:
            out.append([0, n, 1, rank, int(_number('x' + rest[n:])[0]) if len(rest) > n else 0, key[2] if len(key[2]) <= MAX_LEN else None])
        else:
            out.append([1, n, 1, rank, max(0, min(n, contig_len - position)), ''])
    return [tuple(e) for e in out]


# ---- output_from -----------------------------------------------------------------------------------------------------------------
def _tensor_base(x, at):
    t = [int(x[at, b, 1]) + int(x[at, b + 4, 1]) - (int(x[at, b, 3]) + int(x[at, b + 4, 3])) for b in range(4)] + [0, 0, 0, 0]
    return 'ACGT'[int(np.argmax(t)) % 4], sum(t)


def _outcomes(gt, g, v1, v2, ref_base):
    """the lists of possible_outcome_probabilites_from: {name: [(what, float32)]}"""
    o = 16
    vl0 = v1[o] * v2[o]
    L = {'ref': [(None, vl0 * g[0] * gt[GT21.index(ref_base * 2)])],
         'homo_snp': [(k, vl0 * g[1] * gt[k]) for k in HOMO],
         'het_snp': [(k, vl0 * g[2] * gt[k]) for k in HETERO]}
    e = g[1] * gt[15]
    L['homo_ins'] = [(i, v1[o + i] * v2[o + i] * e) for i in range(1, 17)]
    e = g[2] * gt[15]
    L['ins_ins'] = [((min(i, j), max(i, j)), v1[o + i] * v2[o + j] * e) for i in range(1, 17) for j in range(1, 17)]
    L['acgt_ins'] = [((b, i), max(v1[o] * v2[o + i], v1[o + i] * v2[o]) * gt[16 + k] * g[2]) for i in range(1, 17) for k, b in enumerate('ACGT')]
    e = g[1] * gt[10]
    L['homo_del'] = [(i, v1[o - i] * v2[o - i] * e) for i in range(1, 17)]
    e = g[2] * gt[10]
    L['del_del'] = [((min(i, j), max(i, j)), v1[o - i] * v2[o - j] * e) for i in range(1, 17) for j in range(1, 17) if i != j]
    L['acgt_del'] = [((b, i), max(v1[o] * v2[o - i], v1[o - i] * v2[o]) * gt[11 + k] * g[2]) for i in range(1, 17) for k, b in enumerate('ACGT')]
    e = g[2] * gt[20]
    L['ins_del'] = []
    for i in range(1, 17):
        for j in range(1, 17):
            L['ins_del'].append(((j, i), v1[o + i] * v2[o - j] * e))
            L['ins_del'].append(((i, j), v1[o - i] * v2[o + j] * e))
    return L


ORDER = ['ref', 'homo_snp', 'het_snp', 'homo_ins', 'acgt_ins', 'ins_ins', 'homo_del', 'acgt_del', 'del_del', 'ins_del']


def output_from(x, ref, position, probs, sequences, fetch, pysam_all=False, haploid=False, trace=None):
    """-> ((the ten flags), (REF, ALT)).  sequences: the spelled column of the site; fetch(start, end): the FASTA.  trace: a set
    that collects which continuations the loop took."""
    probs = np.asarray(probs, dtype=F32)
    gt, g, v1, v2 = probs[:21], probs[21:24], probs[24:57], probs[57:90]
    centre = ref[FLANK]
    acgt = BASE2ACGT[centre]
    L = _outcomes(gt, g, v1, v2, acgt)
    as_ref = ((True,) + (False,) * 9, (acgt, acgt))

    def hi(v):
        return MAX_LEN if v >= 16 else v

    def insertion(v):
        if pysam_all:
            return insertion_lookup(sequences, v, hi(v))
        if v < 16:
            return ''.join(_tensor_base(x, at)[0] for at in range(FLANK + 1, FLANK + v + 1))
        got = insertion_lookup(sequences, 16, MAX_LEN)
        if got:
            return got
        out = ''
        for at in range(FLANK + 1, 2 * FLANK + 1):
            base, total = _tensor_base(x, at)
            if at < FLANK + 16 or total >= 0.125 * sum(int(x[at, r, 0]) for r in range(8)):
                out += base
            else:
                break
        return out

    def deletion(v):
        if pysam_all:
            return deletion_lookup(sequences, fetch, position, v, hi(v))
        got = deletion_lookup(sequences, fetch, position, 16, MAX_LEN) if v >= 16 else ''
        if not (v >= 16 and len(got) >= FLANK):
            got = ref[FLANK + 1:FLANK + v + 1]
        return got

    def note(what):
        if trace is not None:
            trace.add(what)

    while True:
        top = max(F32(0), max(p for name in ORDER for _, p in L[name]))
        member = {name: any(p == top for _, p in L[name]) for name in ORDER}
        if member['ref']:
            return as_ref
        if haploid and any(member[n] for n in ('het_snp', 'acgt_ins', 'ins_ins', 'acgt_del', 'del_del', 'ins_del')):
            return as_ref
        flags = tuple(member[n] for n in ORDER)
        name = next(n for n in ORDER if member[n])
        if name == 'homo_snp':
            base = 'ACGT'[int(np.argmax([gt[k] for k in HOMO]))]
            return flags, (centre, base)
        if name == 'het_snp':
            b1, b2 = GT21[HETERO[int(np.argmax([gt[k] for k in HETERO]))]]
            if b1 != centre and b2 != centre:
                return flags, (centre, b1 + ',' + b2)
            return flags, (centre, b1 if b1 != centre else b2)
        idx = next(i for i, (_, p) in enumerate(L[name]) if p == top)
        what = L[name].pop(idx)[0]
        if name == 'homo_ins':
            ins = insertion(what)
            if not ins:
                note('nothing')
                continue
            return flags, (centre, centre + ins)
        if name == 'acgt_ins':
            ins = insertion(what[1])
            if not ins:
                note('nothing')
                continue
            alt = centre + ins
            return flags, (centre, what[0] + ',' + alt if what[0] != centre else alt)
        if name == 'ins_ins':
            ins = insertion(what[1])
            if not ins:
                note('nothing')
                continue
            other = insertion_lookup(sequences, what[0], hi(what[0]), ins) or ins[0:what[0]]
            if centre + other != centre + ins:
                return flags, (centre, centre + other + ',' + centre + ins)
            note('ins_ins reset')
            continue
        if name == 'homo_del':
            gone = deletion(what)
            if not gone:
                note('nothing')
                continue
            return flags, (centre + gone, centre)
        if name == 'acgt_del':
            gone = deletion(what[1])
            if not gone:
                note('nothing')
                continue
            if what[0] != centre:
                return flags, (centre + gone, centre + ',' + what[0] + gone)
            return flags, (centre + gone, centre)
        if name == 'del_del':
            gone = deletion(what[1])
            if not gone:
                note('nothing')
                continue
            full = centre + gone
            second = centre + full[what[0] + 1:]
            if centre != second and full != centre and full != second:
                return flags, (full, centre + ',' + second)
            note('del_del reset')
            continue
        ins, gone = insertion(what[1]), deletion(what[0])
        if not ins or not gone:
            note('nothing')
            continue
        return flags, (centre + gone, centre + ',' + centre + ins + gone)


def gt21_of(ref, alt, genotype):
    """gt21_enum_from for the genotype string"""
    alts = alt.split(',')
    if len(alts) == 1:
        alts = [ref if '0' in genotype else alts[0]] + alts
    labels = ['Del' if len(ref) > len(a) else 'Ins' if len(ref) < len(a) else a[0] for a in alts]
    a, b = labels
    if len(a) == 1 and len(b) == 1:
        return GT21.index(min(a, b) + max(a, b))
    if len(a) == 1 or len(b) == 1:
        return GT21.index((a + b) if len(a) == 1 else (b + a))
    return GT21.index(a + b) if a == b else 20


def quality(p, promotion):
    if promotion == 'legacy':
        p = float(p)
        ratio = ((1.0 - p) + 1e-300) / (p + 1e-300)
    else:
        with np.errstate(all='ignore'):
            ratio = float((F32(F32(1.0) - p) + F32(1e-300)) / (p + F32(1e-300)))
    tmp = max((-10 * math.log(math.e, 10)) * math.log(ratio) + 16, 0)
    return int(round(tmp * tmp))


def output_with(chrom, position, ref, x, probs, sequences, fetch, pysam_all=False, haploid=False, show_ref=False, qual=None, promotion='legacy',
                trace=None):
    """one record of the VCF -> (line, its parts), or None.  x: (33, 8, 4) integers."""
    x = np.asarray(x).reshape(33, 8, 4)
    probs = np.asarray(probs, dtype=F32)
    if ref[FLANK] not in 'ACGTU':
        return None
    depth = int(sum(int(x[FLANK, r, 2]) + int(x[FLANK, r, 0]) for r in range(8)))
    if depth == 0:
        return None
    flags, (REF, ALT) = output_from(x, ref, position, probs, sequences, fetch, pysam_all, haploid, trace)
    if (not show_ref and flags[0]) or (not flags[0] and REF == ALT):
        return None
    multi = ',' in ALT
    if flags[0]:
        gts = GENOTYPES[0]
    elif flags[1] or flags[3] or flags[6]:
        gts = GENOTYPES[1]
    elif flags[2] or flags[4] or flags[5] or flags[7] or flags[8]:
        gts = GENOTYPES[2]
    if multi:
        gts = GENOTYPES[3]

    def snp(base):
        n = BASE2NUM[base]
        return int(x[FLANK, n, 3]) + int(x[FLANK, n + 4, 3]) + int(x[FLANK, n, 0]) + int(x[FLANK, n + 4, 0])

    def total(channel):
        return sum(int(x[FLANK + 1, r, channel]) for r in range(8))
    if flags[0]:
        support = int(x[FLANK, BASE2NUM[REF], 0]) + int(x[FLANK, BASE2NUM[REF] + 4, 0])
    elif flags[1] or flags[2]:
        support = sum(snp(b) for b in ALT if b != ',')
    elif flags[3] or flags[5]:
        support = total(1) - total(3)
    elif flags[4]:
        support = total(1) - total(3) + (snp(ALT.split(',')[0][0]) if multi else 0)
    elif flags[6] or flags[8]:
        support = total(2)
    elif flags[7]:
        support = total(2) + (snp(ALT.split(',')[1][0]) if multi else 0)
    else:
        support = total(1) + total(2) - total(3)
    if promotion == 'legacy':
        af = float(support) / float(depth)
    else:
        af = F32(support) / F32(depth)
    if af > 1:
        af = 1
    gt21 = gt21_of(REF, ALT, gts)
    task = {'0/0': 0, '1/1': 1, '0/1': 2, '1/2': 2}[gts]
    p = probs[gt21] * probs[21 + task]
    q = quality(p, promotion)
    filt = '.' if qual is None else ('PASS' if q >= qual else 'LowQual')
    line = '%s\t%d\t.\t%s\t%s\t%d\t%s\t%s\tGT:GQ:DP:AF\t%s:%d:%d:%.4f' % (chrom, position, REF, ALT, q, filt, '.', gts, q, depth, af)
    return line, dict(flags=flags, ref=REF, alt=ALT, gt=gts, gt21=gt21, task=task, p=p, support=support, depth=depth)


def quantize(p):
    """what `%.6f` and numpy's float32 parse leave of float32 values"""
    return np.array(['%.6f' % v for v in np.asarray(p, dtype=F32).reshape(-1).tolist()], dtype=F32).reshape(np.shape(p))
