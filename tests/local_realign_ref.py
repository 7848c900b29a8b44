"""A plain restatement of what megapath_nano_amd/local_realign.py computes: the reference's realignment/local_realignment.py
(-p ont) per site and its extract_vcf_position.py, in Python.  The closed forms of DESIGN.md section 6 item 20:

  members      which records `samtools mpileup -r ctg:pos-233-pos+234 --min-MQ 0 --min-BQ 0` piles up (flags 1796, htslib's overlap,
               the -d 8000 rule: a record is dropped iff it is not the first candidate of its start position and at least maxcnt
               accepted records have end >= its start)
  window       the columns pos-200 .. pos+200 that survive get_nearby_reads (a row with a letter the script does not know is dropped;
               the walk stops at the first missing column after the centre)
  fragment     what a read appends over those columns (ACGT bases under M, = and X; the insertion behind a matched column)
  site         the fragments in dict order, SSW as pyssw.SSW.align calls it, the walk over the SSW CIGAR, depth and the mapping

A read is clair_call_ref's (flag, pos0, [(op, n)], seq).  SSW comes from oracle/ssw_bindings.py (the scalar restatement of ssw.c).
Two forms of a site's fragments:
  * literal: mpileup's text (mpileup_text: htslib's pile-up machine of clair_call_ref with maxcnt, the region filter, `^` + MAPQ and `$`
    marks, `#` for reverse deletions, the quality and name columns) parsed by a restatement of the script's own decode_pileup_bases
    and get_nearby_reads (parse_column, parse_pileup, nearby_reads);
  * closed: members, window, fragment above, which is what the product implements.
tests/test_local_realign_ref.py checks that the two agree on random read sets with maxcnt lowered to 3 .. 6 and on the goldens, which
were recorded from the reference's own programs, the real mpileup included (tests/golden/make_local_realign_golden.py)."""
import json

import numpy as np

import clair_call_ref as ccr

FILTER_FLAG = 1796
MAXCNT = 8000
WINDOW, REGION, REF_FLANK = 200, 233, 300
MAT = np.array([4, -6, -6, -6, 0, -6, 4, -6, -6, 0, -6, -6, 4, -6, 0, -6, -6, -6, 4, 0, 0, 0, 0, 0, 0], dtype=np.int8)
CODE = {'A': 0, 'C': 1, 'G': 2, 'T': 3}


class SiteRaises(Exception):
    """the script raises at this site (its first read has SSW score 0, or its parser meets an indel before a row's first entry)"""


def members(reads, pos, maxcnt=MAXCNT):
    """the indices of the records that the site's mpileup accepts, in file order"""
    beg0, end0 = pos - REGION - 1, pos + REGION + 1
    out, ends, last = [], np.zeros(len(reads), dtype=np.int64), None
    for i, r in enumerate(reads):
        s, e = r[1], r[1] + max(ccr.rlen(r[2]), 1)
        if (r[0] & FILTER_FLAG) or not (s < end0 and e > beg0):
            continue
        first = last is None or s != last
        last = s
        if not first and len(out) >= maxcnt and int(np.count_nonzero(ends[:len(out)] >= s)) >= maxcnt:
            continue
        ends[len(out)] = e
        out.append(i)
    return out


def refuse(read):
    """why the product refuses a record that reaches a site's region, or None"""
    flag, pos0, cigar, seq = read
    if flag & 1:
        return 'paired'
    if seq == '*' or not seq:
        return 'no bases'
    if '=' in seq:
        return 'a base ='
    if any(op in 'NP' for op, _ in cigar):
        return 'N or P'
    if sum(n for op, n in cigar if op in 'MIS=X') > len(seq):
        return 'the CIGAR runs past the bases'
    return None


def window(reads, acc, pos):
    """the surviving columns, 1-based, as a sorted list.  A column exists iff an accepted read covers it and none has a matched base
    there that is not one of ACGTN: mpileup spells such a base as it is, decode_pileup_bases does not know the letter, the counts
    of the row differ and the script drops the row.  The walk stops at the first missing column after the centre."""
    cov, bad = set(), set()
    for i in acc:
        flag, pos0, cigar, seq = reads[i]
        x, y = pos0 + 1, 0
        for op, n in cigar:
            if op in 'MD=X':
                a, b = max(x, pos - WINDOW), min(x + n, pos + WINDOW + 1)
                cov.update(range(a, b))
                if op != 'D':
                    bad.update(p for p in range(a, b) if seq[y + p - x] not in 'ACGTN')
                x += n
            if op in 'MIS=X':
                y += n
    cols = []
    for p in range(pos - WINDOW, pos + WINDOW + 1):
        if p not in cov or p in bad:
            if p > pos:
                break
            continue
        cols.append(p)
    return cols


def entry_at(read, c):
    """does the read give the script's parser an entry at the 0-based column c: a deleted base, or a matched one of ACGTN"""
    flag, pos0, cigar, seq = read
    x, y = pos0, 0
    for op, n in cigar:
        if op in 'MD=X' and x <= c < x + n:
            return op == 'D' or seq[y + c - x] in 'ACGTN'
        if op in 'MDN=X':
            x += n
        if op in 'MIS=X':
            y += n
    return False


def parser_raises(reads, acc, pos):
    """decode_pileup_bases raises IndexError on a row of the region whose first entry would be an indel: a read whose matched stretch
    ends there on a letter the parser does not know (mpileup spells `w+1a`), with an I or a D right behind it, and no read before it
    in the row that gives an entry"""
    for at, i in enumerate(acc):
        flag, pos0, cigar, seq = reads[i]
        x, y = pos0, 0
        for k, (op, n) in enumerate(cigar):
            if op in 'M=X' and n and k + 1 < len(cigar) and cigar[k + 1][0] in 'ID':
                c = x + n - 1
                if pos - REGION - 1 <= c < pos + REGION + 1 and seq[y + n - 1] not in 'ACGTN' and not any(entry_at(reads[j], c) for j in acc[:at]):
                    return True
            if op in 'MDN=X':
                x += n
            if op in 'MIS=X':
                y += n
    return False


def fragment(read, cols):
    """(the text the read appends over the surviving columns, the first column at which it appends) or ('', None)"""
    flag, pos0, cigar, seq = read
    cols = cols if isinstance(cols, (set, frozenset)) else set(cols)
    out, first, x, y, prev = [], None, pos0 + 1, 0, None
    for k, (op, n) in enumerate(cigar):
        if op in 'M=X':
            for j in range(n):
                if x + j in cols and seq[y + j] in 'ACGT':
                    out.append(seq[y + j])
                    first = x + j if first is None else first
            x, y, prev = x + n, y + n, 'M' if n else prev
        elif op == 'I':
            behind = next((o for o, l in cigar[k + 1:] if o != 'I'), None)      # `+2AA-3NNN`: the script keeps the deletion only
            if prev == 'M' and x - 1 in cols and behind != 'D':
                out.append(seq[y:y + n].upper())
                first = x - 1 if first is None else first
            y += n
        elif op == 'D':
            x, prev = x + n, 'D' if n else prev
        elif op == 'S':
            y, prev = y + n, 'S'
        elif op == 'H':
            prev = 'H'
    return ''.join(out), first


def fragments_of(reads, pos, maxcnt=MAXCNT):
    """[(index of the read, its fragment)] of a site in the order of the script's dict, by the closed forms"""
    acc = members(reads, pos, maxcnt)
    if parser_raises(reads, acc, pos):
        raise SiteRaises(pos)
    cols = set(window(reads, acc, pos))
    got = []
    for i in acc:
        text, first = fragment(reads[i], cols)
        if text:
            got.append((first, i, text))
    got.sort(key=lambda g: (g[0], g[1]))
    return [(g[1], g[2]) for g in got]


def fragments(reads, pos, maxcnt=MAXCNT, literal=False):
    """the fragments of a site in the order of the script's dict"""
    return [f for _, f in (literal_fragments_of if literal else fragments_of)(reads, pos, maxcnt)]


# ---- the literal form: mpileup's text, and the script's own parse of it ---------------------------------------------------------------
def mpileup_text(reads, pos, maxcnt=MAXCNT, ctg='ctg', mapq=60):
    """What `samtools mpileup -r ctg:pos-233-pos+234 --reverse-del --min-MQ 0 --min-BQ 0 --output-QNAME` (no -f) prints: htslib's
    pile-up machine (clair_call_ref.Pileup with this maxcnt) over the records that pass the flag filter and overlap the region, and
    per column of the region the spelling of pileup_seq -- `^` and the MAPQ character before a read's first base, `$` behind its
    last, the base as it stands (an IUPAC letter stays one), lower case on the reverse strand, `*` or, reverse, `#` for a deleted
    base, `>` `<` for a skipped one, `+2AA` for an insertion, `-3NNN` for a deletion, and `+2AA-3NNN` for both -- a quality
    character per read and the names (the read's index, as `r<index>`)."""
    beg0, end0 = pos - REGION - 1, pos + REGION + 1
    name = {}
    taken = []
    for i, r in enumerate(reads):
        if not (r[0] & FILTER_FLAG) and r[1] < end0 and r[1] + max(ccr.rlen(r[2]), 1) > beg0:
            name[id(r)] = 'r%d' % i
            taken.append(r)
    plp, out = ccr.Pileup(taken, maxcnt=maxcnt), []
    while True:
        got = plp.auto()
        if got is None:
            break
        at, column = got
        if not beg0 <= at < end0:
            continue
        bases, quals, names = '', '', []
        for read, k, x, y in column:
            if k < 0:
                continue
            text = ccr.spell(read, k, x, y, at)
            if text[0] == '*' and read[0] & 16:
                text = '#' + text[1:]
            if at == read[1]:
                text = '^' + chr(min(mapq, 93) + 33) + text
            if at == read[1] + ccr.rlen(read[2]) - 1:
                text += '$'
            bases, quals = bases + text, quals + 'I'
            names.append(name[id(read)])
        out.append('\t'.join([ctg, str(at + 1), 'N', str(len(names)), bases, quals, ','.join(names)]) + '\n')
    return ''.join(out)


def parse_column(text):
    """the script's decode_pileup_bases: -> [[base, indel]].  It knows the letters ACGTNacgtn#*; `^` hides the next character; an
    indel text replaces what the entry before it had, so a deletion spelled behind an insertion takes its place; anything else
    (`$`, an IUPAC letter, `<` `>`) is passed over without an entry."""
    out, i = [], 0
    while i < len(text):
        c = text[i]
        if c in '+-':
            j = i + 1
            while text[j].isdigit():
                j += 1
            n = int(text[i + 1:j])
            out[-1][1] = c + text[j:j + n]
            i = j + n
        elif c in 'ACGTNacgtn#*':
            out.append([c, ''])
            i += 1
        else:
            i += 2 if c == '^' else 1
    return out


def parse_pileup(text):
    """the script's loop over mpileup's rows: -> {position: (names, entries)}; a row whose names or qualities do not count as many
    as its entries is dropped"""
    table = {}
    for row in text.splitlines():
        col = row.strip().split('\t')
        entries, names = parse_column(col[4]), col[6].split(',')
        if len(names) == len(entries) == len(col[5]):
            table[int(col[1])] = (names, entries)
    return table


def nearby_reads(centre, table):
    """the script's get_nearby_reads: -> {name: fragment} in the order in which the names first get text"""
    frag = {}
    for p in range(centre - WINDOW, centre + WINDOW + 1):
        if p not in table:
            if p > centre:
                break
            continue
        for who, (base, indel) in zip(*table[p]):
            if base in '#*':
                continue
            if base.upper() in 'ACGT':
                frag[who] = frag.get(who, '') + base.upper()
            if indel and indel[0] == '+':
                frag[who] = frag.get(who, '') + indel[1:].upper()
    return frag


def literal_fragments_of(reads, pos, maxcnt=MAXCNT):
    """[(index of the read, its fragment)] in the order of the script's dict, through the text"""
    try:
        table = parse_pileup(mpileup_text(reads, pos, maxcnt))
    except IndexError:                      # (parse_column: an indel text before the row's first entry)
        raise SiteRaises(pos)
    return [(int(who[1:]), f) for who, f in nearby_reads(pos, table).items()]


def ref_window(contig, pos):
    """contig[pos-301 : pos+300] as Python slices it (pos > 300), upper case"""
    return contig[pos - REF_FLANK - 1:pos + REF_FLANK].upper()


def oracle_ssw(query, ref):
    from oracle.ssw_bindings import oracle_align
    q = np.array([CODE.get(c, 4) for c in query], dtype=np.int8)
    r = np.array([CODE.get(c, 4) for c in ref], dtype=np.int8)
    return oracle_align(read=q, ref=r, mat=MAT, gap_open=8, gap_extend=2, flag=2, filters=0, filterd=0, mask=15 if len(q) <= 30 else len(q),
                        score_size=2)


def get_cigar(res, query):
    """pyssw.SSW.get_cigar"""
    score, _, rb, re_, qb, qe, _, cigar = res
    text = ''
    if qb > 0:
        text += str(qb) + 'S'
    for x in cigar:
        n, m = x >> 4, x & 15
        c = 'M' if m > 8 else 'MIDNSHP=X'[m]
        text += str(n) + ('=' if c == 'M' else c)
    if qe - qb + 1 < len(query):
        text += str(len(query) - (qe - qb + 1)) + 'S'
    return text


def site(reads, contig, pos, ssw=oracle_ssw, maxcnt=MAXCNT, detail=None, keep_ref=False, literal=False):
    """-> (depth, the ordered mapping) of a 1-based site with pos > 300; SiteRaises where the script raises.  keep_ref: the contig's own
    base stays in the mapping (what the device hands to the host)."""
    frags = fragments(reads, pos, maxcnt, literal)
    ref = ref_window(contig, pos)
    upper = contig.upper()
    info, ref_pos = [], None
    for f in frags:
        res = ssw(f, ref) if ref else None
        score = res[0] if isinstance(res, tuple) else 0
        if score > 0:
            ref_pos = res[2] + pos - REF_FLANK
        if ref_pos is None:
            raise SiteRaises(pos)
        info.append((f, get_cigar(res, f) if score > 0 else '', ref_pos))
        if detail is not None:
            detail.append((f, res))
    info.sort(key=lambda x: x[2])
    alt = {}
    for seq, cigar, r in info:
        ops = ccr.parse_cigar(cigar)
        clip_end = ops[-1][1] if len(ops) > 1 and ops[-1][0] == 'S' else 0
        ops = [o for o in ops if o[0] != 'S']
        if clip_end > 0:
            seq = seq[:-clip_end]
        q = 0
        for op, n in ops:
            if op in 'M=X':
                if pos >= r and r + n > pos and q + pos - r < len(seq):
                    k = seq[q + pos - r]
                    alt[k] = alt.get(k, 0) + 1
                r, q = r + n, q + n
            elif op == 'I':
                if pos == r - 1:
                    k = 'I' + seq[q:q + n].upper()
                    alt[k] = alt.get(k, 0) + 1
                q += n
            elif op == 'D':
                if pos == r - 1:
                    k = 'D' + upper[r - 1:r - 1 + n]
                    alt[k] = alt.get(k, 0) + 1
                r += n
    depth = sum(c for k, c in alt.items() if k[0] not in 'ID')
    if not keep_ref:
        alt.pop(upper[pos - 1], None)
    return depth, alt


def line(ctg, pos, depth, alt):
    return '\t'.join([ctg, str(pos), str(depth), json.dumps(alt), str(pos)]) + '\n'


def lines(reads, contig, ctg, positions, ssw=oracle_ssw, maxcnt=MAXCNT, literal=False):
    """the lines of local_realign.local_realignment: a site with pos <= 300 and one at which the script raises are left out"""
    out = []
    for pos in sorted(set(positions)):
        if pos <= REF_FLANK:
            continue
        try:
            out.append(line(ctg, pos, *site(reads, contig, pos, ssw, maxcnt, literal=literal)))
        except SiteRaises:
            pass
    return ''.join(out)


# ---- extract_vcf_position.py ----------------------------------------------------------------------------------------------------
def find_af(depth, alt, ref_base, alt_base):
    count = 0
    if len(ref_base) == len(alt_base) == 1:
        count = int(alt.get(alt_base, 0))
    elif len(ref_base) < len(alt_base):
        count = int(alt.get('I' + alt_base[1:], 0))
    elif len(ref_base) > len(alt_base):
        count = int(alt.get('D' + ref_base[1:], 0))
    return count / float(depth) if count > 0 else None


def extract_vcf_position(vcf_text, alt_text):
    """-> (the text of the output VCF, the text of standard output)"""
    alts = {}
    for ln in alt_text.rstrip().split('\n'):
        f = ln.rstrip().split('\t')
        alts[f[0] + ' ' + str(int(f[1]))] = (int(f[2]), json.loads(f[3]))
    out, said = [], []
    for row in vcf_text.splitlines():
        row = row.rstrip()
        if row[0] == '#':
            out.append(row)
            continue
        col = row.strip().split('\t')
        key = col[0] + ' ' + str(int(col[1]))
        if key in alts:
            gt, gq, _, _ = col[-1].split(':')
            dp, alt = alts[key]
            af = find_af(dp, alt, col[3], col[4])
            if af and af > 0:
                said.append('[INFO] {}:{} updates allele frequency to {}\n'.format(col[0], int(col[1]), round(af, 4)))
                row = '\t'.join(col[:-1] + ['%s:%s:%d:%.4f' % (gt, gq, dp, af)])
            out.append(row)
    # (the script orders the header before the records)
    head = [r for r in out if r[0] == '#']
    return '\n'.join(head + [r for r in out if r[0] != '#']), ''.join(said)
