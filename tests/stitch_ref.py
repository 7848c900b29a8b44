"""Plain sequential restatement of the stitching stage (csrc/stitch_kernels.h: stitch_kernel): the second half of minimap2's mm_align1
-- the windows' CIGARs appended in order with mm_append_cigar's merge rule, the DP score, the end coordinates, the cut at the first
gap fill that z-dropped or got no DP, the search for the anchor the hit is split at, and mm_split_reg's measures of the two halves --
in Python integers and lists.  test_stitch_ref.py pins it to the oracle's own function (mmo_stitch_hit, the code align1 runs);
test_ext_stitch_gpu.py compares the kernel with it.

Nothing here is shaped like the kernel: one pass over the windows in order, one growing list of [kind, length] operations.
stitch_ref() also returns what happened on the way (`ev`), so that the tests can assert that their cases reach the mechanisms they
were written for.

A window is a dict: flag, reversed, qs, ts, anchor (plan_ref's window fields) and its result res = dict(max, zdropped, max_q, max_t,
mqe_t, score, reach_end, ops [(kind, length)]).  The result of a placeholder (flag & EZ_REFUSED) is never looked at."""
from plan_ref import EZ_EXTZ_ONLY, EZ_REFUSED, ax, ay, span

EZ_INV = 0x200
OUT_KEYS = ('n_ops', 'dp_score', 'rs1', 're1', 'qs1', 'qe1', 'has_p', 'dropped', 'drop_fill', 'drop_max_t', 'drop_max_q', 'split_n',
            'split_inv')
FIN_KEYS = ('n_cigar', 'read', 'rid', 'rev', 'qs1', 'rs1', 'qspan', 'tspan')
REFUSED_RES = dict(max=0, zdropped=1, max_q=-1, max_t=-1, mqe_t=-1, score=0, reach_end=0, ops=[])   # align_pair's answer without DP


def new_ev():
    return dict(merges=0, merges_through_single=0, max_adds_on_one_op=0, empty_skipped=[], merge_joins=[], cut=None, steps=None,
                fell_through=False, margin=None, ext_zdropped=0, ext_max_not_counted=0, drop_uses_max=False, refused=[])


def fuzzy(a):
    """mm_cal_fuzzy_len over the anchors a -> (mlen, blen)"""
    mlen = blen = span(a[0])
    for p, c in zip(a, a[1:]):
        tl, ql = ax(c) - ax(p), ay(c) - ay(p)
        blen += max(tl, ql)
        mlen += span(c) if tl > span(c) and ql > span(c) else min(tl, ql)
    return mlen, blen


def stitch_hit(a, hit, wins, min_cnt, read=0):
    """a: the read's anchors [(x, y)]; hit: as, cnt, as1, cnt1, qs, rs, qe, re, qs0, qe0, rid, rev (plan_ref's hit record and the hit's
    own as / cnt); wins: its windows in order -> (out dict: OUT_KEYS, cigar [op words], fin dict of FIN_KEYS, split dict or None), ev"""
    ev = new_ev()
    cigar = []                      # [kind, length]
    adds = []                       # per op: how many windows' first ops were added to it
    last_nonempty, since_nonempty, last_was_single_merged = None, 0, False
    dp = 0
    has_p = dropped = 0
    rs1, qs1, re1, qe1 = hit['rs'], hit['qs'], hit['re'], hit['qe']
    out = dict(drop_fill=-1, drop_max_t=-1, drop_max_q=-1, split_n=0, split_inv=0)
    split = None
    n_fill = 0

    def append(k, ops):
        nonlocal has_p, last_nonempty, since_nonempty, last_was_single_merged
        if not ops:
            since_nonempty += 1
            return
        has_p = 1
        merged = bool(cigar) and cigar[-1][0] == ops[0][0]
        if merged:
            cigar[-1][1] += ops[0][1]
            adds[-1] += 1
            ev['merges'] += 1
            ev['merge_joins'].append((last_nonempty, k))
            ev['empty_skipped'].append(since_nonempty)
            if last_was_single_merged:
                ev['merges_through_single'] += 1
            ev['max_adds_on_one_op'] = max(ev['max_adds_on_one_op'], adds[-1])
            rest = ops[1:]
        else:
            rest = ops
        for kind, length in rest:
            cigar.append([kind, length])
            adds.append(0)
        last_was_single_merged = merged and len(ops) == 1
        last_nonempty, since_nonempty = k, 0

    for k, w in enumerate(wins):
        refused = bool(w['flag'] & EZ_REFUSED)
        r = REFUSED_RES if refused else w['res']
        if refused:
            ev['refused'].append(k)
        if w['flag'] & EZ_EXTZ_ONLY:
            left = bool(w['reversed'])
            assert k == (0 if left else len(wins) - 1)
            if not refused and r['zdropped']:
                ev['ext_zdropped'] += 1
            append(k, r['ops'])
            if r['ops']:
                dp += r['max']
            elif r['max'] > 0:
                ev['ext_max_not_counted'] += 1
            if left:
                rs1 = hit['rs'] - (r['mqe_t'] + 1 if r['reach_end'] else r['max_t'] + 1)
                qs1 = hit['qs'] - (hit['qs'] - hit['qs0'] if r['reach_end'] else r['max_q'] + 1)
            else:
                re1 = hit['re'] + (r['mqe_t'] + 1 if r['reach_end'] else r['max_t'] + 1)
                qe1 = hit['qe'] + (hit['qe0'] - hit['qe'] if r['reach_end'] else r['max_q'] + 1)
            continue
        append(k, r['ops'])
        if not r['zdropped']:
            dp += r['score']
            n_fill += 1
            continue
        # ---- the alignment broke in this fill: the hit ends here
        has_p = dropped = 1
        ev['cut'] = k
        ev['drop_uses_max'] = r['max'] != r['score']
        dp += r['max']
        as1, cnt1 = hit['as1'], hit['cnt1']
        j, steps = w['anchor'] - 1, 0
        while j >= 0 and not ax(a[as1 + j]) <= w['ts'] + r['max_t']:
            j -= 1
            steps += 1
        ev['steps'] = steps
        if j < 0:
            j = 0
            ev['fell_through'] = True
        re1, qe1 = w['ts'] + r['max_t'] + 1, w['qs'] + r['max_q'] + 1
        out.update(drop_fill=n_fill, drop_max_t=r['max_t'], drop_max_q=r['max_q'])
        ev['margin'] = cnt1 - (j + 1) - min_cnt
        if cnt1 - (j + 1) >= min_cnt:
            n = as1 + j + 1 - hit['as']
            out['split_n'] = n
            out['split_inv'] = 1 if w['flag'] & EZ_INV else 0
            if 0 < n < hit['cnt']:      # (mm_split_reg does nothing for a cut outside the hit)
                h = a[hit['as']:hit['as'] + hit['cnt']]
                ml, bl = fuzzy(h[:n])
                mr, br = fuzzy(h[n:])
                split = dict(fx=h[n][0], fy=h[n][1], lx_left=h[n - 1][0], ly_left=h[n - 1][1], mlen_l=ml, blen_l=bl, mlen_r=mr, blen_r=br,
                             r2_as=hit['as'] + n, r2_cnt=hit['cnt'] - n)
        break
    words = [length << 4 | kind for kind, length in cigar]
    out.update(n_ops=len(words), dp_score=dp, rs1=rs1, re1=re1, qs1=qs1, qe1=qe1, has_p=has_p, dropped=dropped)
    fin = dict(n_cigar=len(words), read=read, rid=hit['rid'], rev=hit['rev'], qs1=qs1, rs1=rs1, qspan=max(qe1 - qs1, 0), tspan=max(re1 - rs1, 0))
    return (out, words, fin, split), ev
