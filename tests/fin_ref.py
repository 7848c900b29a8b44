"""Plain sequential restatement of what the finishing kernel computes (csrc/fin_kernels.h): minimap2's mm_fix_cigar followed by
mm_update_extra on one alignment, written from the algorithm's statement with Python lists and no parallel re-derivation.

  fix:    every gap between two match runs moves left while the base before it equals the gap's last base (the match run before
          it shrinks, the one after it grows; a later gap sees the grown run); runs of adjacent insertions and deletions (with
          empty ops among them) of more than two ops and both kinds become one I and one D; empty ops are dropped and equal
          neighbours joined when any of this left an empty op; a leading gap is removed and moves the alignment's start.
  extra:  blen / mlen / n_ambi over the columns, dp_max the maximum of the running score clipped at 0.

fin_ref() also returns what happened on the way (`ev`), so that the tests can assert that their cases reach the mechanisms the
kernel treats specially: gaps that eat the whole run before them, those among them that needed what gap k-2 had moved in, merges,
shrinks, leading gaps."""

M, I, D = 0, 1, 2


def op(n, o):
    return n << 4 | o


def fin_ref(cigar, q, t, a=2, b=4, sc_ambi=1, q_=4, e=2):
    """cigar: words len << 4 | op (ops 0..2); q, t: 0..4 codes in alignment orientation -> dict(n_cigar, qshift, tshift, blen,
    mlen, n_ambi, dp_max, cigar, ev)"""
    ops = [c & 15 for c in cigar]
    lens = [c >> 4 for c in cigar]
    orig = list(lens)
    n = len(ops)
    q = [int(x) for x in q]
    t = [int(x) for x in t]
    ev = dict(shifted=0, saturated=0, dependent=0, dependent_at=[], merged=0, shrinks=0, lead_i=0, lead_d=0, max_shift=0)
    qshift = tshift = 0
    if n > 1:
        shrink = False
        qoff = toff = 0
        for k in range(n):
            o, ln = ops[k], lens[k]
            if ln == 0:
                shrink = True
            if o == M:
                qoff += ln
                toff += ln
                continue
            if 0 < k < n - 1 and ops[k - 1] == M and ops[k + 1] == M:
                seq, off = (q, qoff) if o == I else (t, toff)
                prev = lens[k - 1]           # what gap k-2 moved into the run is part of it by now
                s = 0
                while s < prev and seq[off - 1 - s] == seq[off + ln - 1 - s]:
                    s += 1
                if s > 0:
                    lens[k - 1] -= s
                    lens[k + 1] += s
                    qoff -= s
                    toff -= s
                    ev['shifted'] += 1
                    ev['max_shift'] = max(ev['max_shift'], s)
                if s == prev:
                    shrink = True
                if s >= orig[k - 1]:
                    ev['saturated'] += 1
                if s > orig[k - 1]:
                    ev['dependent'] += 1
                    ev['dependent_at'].append(k)
            if o == I:
                qoff += ln
            else:
                toff += ln
        k = 0
        while k < n - 2:
            if ops[k] != M and ops[k] + ops[k + 1] == 3:
                tot = [0, 0, 0]
                j = k
                while j < n and (ops[j] != M or lens[j] == 0):
                    tot[ops[j]] += lens[j]
                    j += 1
                if tot[I] > 0 and tot[D] > 0 and j - k > 2:
                    ops[k], lens[k] = I, tot[I]
                    ops[k + 1], lens[k + 1] = D, tot[D]
                    for x in range(k + 2, j):
                        lens[x] = 0
                    shrink = True
                    ev['merged'] += 1
                k = j
            k += 1
        if shrink:
            ev['shrinks'] += 1
            kept = [(o, ln) for o, ln in zip(ops, lens) if ln != 0]
            joined = []
            for o, ln in kept:
                if joined and joined[-1][0] == o:
                    joined[-1][1] += ln
                else:
                    joined.append([o, ln])
            ops, lens = [x[0] for x in joined], [x[1] for x in joined]
            n = len(ops)
        if n > 0 and ops[0] != M:
            if ops[0] == I:
                qshift = lens[0]
                ev['lead_i'] += 1
            else:
                tshift = lens[0]
                ev['lead_d'] += 1
            ops, lens = ops[1:], lens[1:]
            n -= 1
    blen = mlen = n_ambi = 0
    s = dp_max = 0
    qoff, toff = qshift, tshift
    for o, ln in zip(ops, lens):
        if o == M:
            for x in range(ln):
                cq, ct = q[qoff + x], t[toff + x]
                if cq > 3 or ct > 3:
                    n_ambi += 1
                    s -= sc_ambi
                elif cq == ct:
                    mlen += 1
                    blen += 1
                    s += a
                else:
                    blen += 1
                    s -= b
                if s < 0:
                    s = 0
                elif s > dp_max:
                    dp_max = s
            qoff += ln
            toff += ln
        else:
            seq, off = (q, qoff) if o == I else (t, toff)
            amb = sum(1 for x in range(ln) if seq[off + x] > 3)
            blen += ln - amb
            n_ambi += amb
            s = max(0, s - (q_ + e * ln))
            if o == I:
                qoff += ln
            else:
                toff += ln
    return dict(n_cigar=n, qshift=qshift, tshift=tshift, blen=blen, mlen=mlen, n_ambi=n_ambi, dp_max=dp_max,
                cigar=[ln << 4 | o for o, ln in zip(ops, lens)], ev=ev)


KEYS = ('n_cigar', 'qshift', 'tshift', 'blen', 'mlen', 'n_ambi', 'dp_max', 'cigar')
