"""Reference writer of the cs / MD strings and the =/X CIGAR (test infrastructure, written from the definition in
include/mpn_map.h and DESIGN.md section 6): a plain loop over the columns of one alignment.

An alignment is (CIGAR ops as len << 4 | op with op 0 M, 1 I, 2 D; the read slice in the alignment's orientation and the target
slice, both as 0..4 codes).  A column of an M op matches iff the two codes are equal (N against N matches)."""
import re

import numpy as np

LO, UP = 'acgtn', 'ACGTN'
CS, CS_LONG, MD, EQX = 1, 2, 4, 8

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate('ACGT'):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def codes(seq):
    """ASCII (bytes / str / uint8 array) -> 0..4 codes; anything that is not ACGT in either case is 4"""
    if isinstance(seq, str):
        seq = seq.encode()
    return _CODE[np.frombuffer(bytes(seq), dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)]


def revcomp_codes(c):
    c = np.asarray(c, dtype=np.uint8)[::-1]
    return np.where(c < 4, 3 - c, 4).astype(np.uint8)


def parse_cigar(text):
    return [int(n) << 4 | 'MIDNSHP=X'.index(o) for n, o in re.findall(r'(\d+)([MIDNSHP=X])', text)]


def cigar_text(ops):
    return ''.join('%d%s' % (c >> 4, 'MIDNSHP=X'[c & 15]) for c in ops)


def collapse_eqx(ops):
    """=/X ops back to M, neighbours merged"""
    out = []
    for c in ops:
        op = 0 if (c & 15) in (7, 8) else c & 15
        if out and (out[-1] & 15) == op == 0:
            out[-1] += c >> 4 << 4
        else:
            out.append(c >> 4 << 4 | op)
    return out


def write_tags(cigar, q, t):
    """-> dict(cs, cs_long, md, eqx).  An alignment without ops has no strings."""
    if not len(cigar):
        return dict(cs='', cs_long='', md='', eqx=[])
    q, t = [int(x) for x in q], [int(x) for x in t]
    cs, csl, md, eqx = [], [], [], []
    qi = ti = 0
    md_n = 0
    for c in cigar:
        ln, op = int(c) >> 4, int(c) & 15
        if op == 0:
            run = []                    # the open run of matching columns (never continues across an op)
            e_op, e_len = None, 0       # the open = or X op

            def flush():
                if run:
                    cs.append(':%d' % len(run))
                    csl.append('=' + ''.join(run))
                    del run[:]
            for _ in range(ln):
                a, b = t[ti], q[qi]
                if a == b:
                    run.append(UP[a])
                    md_n += 1
                    cur = 7
                else:
                    flush()
                    x = '*' + LO[a] + LO[b]
                    cs.append(x)
                    csl.append(x)
                    md.append('%d%s' % (md_n, UP[a]))
                    md_n = 0
                    cur = 8
                if cur == e_op:
                    e_len += 1
                else:
                    if e_op is not None:
                        eqx.append(e_len << 4 | e_op)
                    e_op, e_len = cur, 1
                qi += 1
                ti += 1
            flush()
            if e_op is not None:
                eqx.append(e_len << 4 | e_op)
        elif op == 1:
            x = '+' + ''.join(LO[v] for v in q[qi:qi + ln])
            cs.append(x)
            csl.append(x)
            eqx.append(ln << 4 | 1)
            qi += ln
        elif op == 2:
            x = ''.join(LO[v] for v in t[ti:ti + ln])
            cs.append('-' + x)
            csl.append('-' + x)
            md.append('%d^%s' % (md_n, x.upper()))
            md_n = 0
            eqx.append(ln << 4 | 2)
            ti += ln
        else:
            raise ValueError('op %d' % op)
    assert qi == len(q) and ti == len(t), (qi, len(q), ti, len(t))
    md.append('%d' % md_n)
    return dict(cs=''.join(cs), cs_long=''.join(csl), md=''.join(md), eqx=eqx)


MD_RE = re.compile(r'^[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*$')


def replay_cs(cs, t_letters):
    """the read slice (upper case, in the alignment's orientation) that a cs string, short or long, makes of the target slice"""
    out, ti = [], 0
    for m in re.finditer(r':(\d+)|=([A-Z]+)|\*([a-z])([a-z])|\+([a-z]+)|-([a-z]+)', cs):
        if m.group(1) is not None:
            k = int(m.group(1))
            out.append(t_letters[ti:ti + k])
            ti += k
        elif m.group(2) is not None:
            assert t_letters[ti:ti + len(m.group(2))] == m.group(2)
            out.append(m.group(2))
            ti += len(m.group(2))
        elif m.group(3) is not None:
            assert t_letters[ti] == m.group(3).upper()
            out.append(m.group(4).upper())
            ti += 1
        elif m.group(5) is not None:
            out.append(m.group(5).upper())
        else:
            assert t_letters[ti:ti + len(m.group(6))] == m.group(6).upper()
            ti += len(m.group(6))
    assert ti == len(t_letters), (ti, len(t_letters))
    assert sum(len(m.group(0)) for m in re.finditer(r':(\d+)|=([A-Z]+)|\*([a-z])([a-z])|\+([a-z]+)|-([a-z]+)', cs)) == len(cs)
    return ''.join(out)


def replay_md(md, cigar, q_letters):
    """the target slice that MD + CIGAR (M or =/X form) + the read slice (upper case, alignment orientation) give"""
    assert MD_RE.match(md), md[:80]
    items = re.findall(r'(\d+)|\^([A-Z]+)|([A-Z])', md)
    # expand MD to a stream over the target-consuming columns: ('=',) match, ('X', base) mismatch, ('D', base) deleted
    stream = []
    for num, dele, mis in items:
        if num:
            stream.extend('=' * int(num))
        elif dele:
            stream.extend(('D', b) for b in dele)
        else:
            stream.append(('X', mis))
    out, qi, si = [], 0, 0
    for c in cigar:
        ln, op = c >> 4, c & 15
        if op in (0, 7, 8):
            for _ in range(ln):
                s = stream[si]
                si += 1
                out.append(q_letters[qi] if s == '=' else s[1])
                assert s == '=' or s[0] == 'X'
                qi += 1
        elif op == 1:
            qi += ln
        elif op == 2:
            for _ in range(ln):
                s = stream[si]
                si += 1
                assert s != '=' and s[0] == 'D'
                out.append(s[1])
    assert si == len(stream) and qi == len(q_letters)
    return ''.join(out)


def letters(c):
    return ''.join(UP[int(x)] for x in c)
