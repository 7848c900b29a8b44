"""Plain sequential restatement of the extension planning stage (csrc/plan_kernels.h: plan_kernel, plan_hit, pk_filter_bad_seeds):
the first half of minimap2's mm_align1 -- mm_fix_bad_ends, mm_filter_bad_seeds, the limits of the two end extensions and the cut
of a hit into left extension, gap fills and right extension -- on one read's squeezed anchors, in Python integers.
test_plan_ref.py pins it to the oracle's own functions (mmo_plan_hit); test_ext_plan_gpu.py compares the kernel with it.

Nothing here is shaped like the kernel: the read's anchors are one flat list of [x, y] words, the K list of mm_filter_bad_seeds is
an explicit list of indices, and a hit is planned in one pass.  plan_ref() also returns what happened on the way (`ev`), so that
the tests can assert that their cases reach the mechanisms they were written for.

A window that max_sw_mat refuses is kept as a placeholder, the record format of the stage (csrc/stitch_kernels.h): its start
coordinates, its flags | EZ_REFUSED and its place in the hit stay; lengths, band, z-drop and end bonus are 0.  `raw` keeps what
the window would have been (what the oracle's align_pair is handed)."""
M32 = (1 << 32) - 1
SEED_LONG_JOIN, SEED_IGNORE, SEED_TANDEM = 1 << 40, 1 << 41, 1 << 42
EZ_APPROX_MAX, EZ_RIGHT, EZ_EXTZ_ONLY, EZ_REV_CIGAR, EZ_REFUSED = 0x02, 0x08, 0x40, 0x80, 0x100
DEFAULTS = dict(bw=500, min_chain_score=40, max_gap=5000, min_cnt=3, a=2, q=4, e=2, zdrop=400, zdrop_inv=200, end_bonus=-1, min_ksw_len=200,
                max_sw_mat=100000000)
HIT_KEYS = ('n_jobs', 'as1', 'cnt1', 'qs', 'rs', 'qe', 're', 'qs0', 'qe0', 'rid', 'rev')
WIN_KEYS = ('rid', 'rev', 'qs', 'qlen', 'ts', 'tlen', 'reversed', 'w', 'zdrop', 'end_bonus', 'flag', 'anchor')
# mm_align1's call of mm_filter_bad_seeds
MIN_GAP, DIFF_THRES, MAX_EXT_CNT = 10, 40, 10


def i32(v):
    """the low 32 bits of v as a signed int: (int32_t)v"""
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def ax(p):
    return i32(p[0])


def ay(p):
    return i32(p[1])


def span(p):
    return p[1] >> 32 & 0xff


def cdiv(n, d):
    """n / d of C: towards zero"""
    q = abs(n) // abs(d)
    return q if (n < 0) == (d < 0) else -q


def fix_bad_ends(o, a, as_, cnt, mlen, ev):
    as1, cnt1 = as_, cnt
    if cnt < 3:
        return as1, cnt1
    bw, min_match = o['bw'], o['min_chain_score'] * 2

    def stop(l, m):       # the first of the three conditions that holds, as C's || evaluates them
        if l >= bw << 1:
            return 'l'
        if m >= min_match and m >= bw:
            return 'm'
        if m >= mlen >> 1:
            return 'mlen'
        return None

    m = l = span(a[as_])
    why = 'end'
    for i in range(as_ + 1, as_ + cnt - 1):
        if a[i][1] & SEED_LONG_JOIN:
            why = 'long_join'
            break
        lr, lq = ax(a[i]) - ax(a[i - 1]), ay(a[i]) - ay(a[i - 1])
        mn, mx = min(lr, lq), max(lr, lq)
        if mx - mn > l >> 1:
            as1 = i
        l += mn
        m += min(mn, span(a[i]))
        why = stop(l, m)
        if why:
            break
        why = 'end'
    ev['front_stop'] = why
    cnt1 = as_ + cnt - as1
    m = l = span(a[as_ + cnt - 1])
    why = 'end'
    for i in range(as_ + cnt - 2, as1, -1):
        if a[i + 1][1] & SEED_LONG_JOIN:
            why = 'long_join'
            break
        lr, lq = ax(a[i + 1]) - ax(a[i]), ay(a[i + 1]) - ay(a[i])
        mn, mx = min(lr, lq), max(lr, lq)
        if mx - mn > l >> 1:
            cnt1 = i + 1 - as1
        l += mn
        m += min(mn, span(a[i + 1]))
        why = stop(l, m)
        if why:
            break
        why = 'end'
    ev['back_stop'] = why
    return as1, cnt1


def filter_bad_seeds(a, as1, cnt1, max_ext_len, ev):
    def gap(i):
        return (ay(a[as1 + i]) - ay(a[as1 + i - 1])) - (ax(a[as1 + i]) - ax(a[as1 + i - 1]))

    K = [i for i in range(1, cnt1) if gap(i) < -MIN_GAP or gap(i) > MIN_GAP]
    ev['K'] = K
    n = len(K)
    if n <= 1:
        return
    mx, max_st, max_en = 0, -1, -1
    k = 0
    while True:
        if k == n or k >= max_en:
            if max_en > 0:
                for i in range(K[max_st], K[max_en]):
                    a[as1 + i][1] |= SEED_IGNORE
                ev['ranges'].append((K[max_st], K[max_en]))
            mx, max_st, max_en = 0, -1, -1
            if k == n:
                break
        i = K[k]
        n_ins = n_del = 0
        g = gap(i)
        if g > 0:
            n_ins += g
        else:
            n_del += -g
        qs, rs = ay(a[as1 + i - 1]), ax(a[as1 + i - 1])
        max_diff, max_diff_l = 0, -1
        l = k + 1
        while l < n and l <= k + MAX_EXT_CNT:
            j = K[l]
            if ay(a[as1 + j]) - qs > max_ext_len or ax(a[as1 + j]) - rs > max_ext_len:
                ev['ext_len_breaks'] += 1
                break
            g = gap(j)
            if g > 0:
                n_ins += g
            else:
                n_del += -g
            diff = n_ins + n_del - abs(n_ins - n_del)
            if max_diff < diff:
                max_diff, max_diff_l = diff, l
            l += 1
        else:
            if l < n:
                ev['ext_cnt_breaks'] += 1      # more K entries lay ahead than max_ext_cnt lets a run take
        ev['max_diffs'].append(max_diff)
        if max_diff > DIFF_THRES and max_diff > mx:
            if max_en > 0:
                ev['range_replaced'] += 1      # a larger maximum while inside an earlier range: that one is never marked
            mx, max_st, max_en = max_diff, k, max_diff_l
        k += 1


def new_ev():
    return dict(front_stop=None, back_stop=None, K=[], ranges=[], ext_len_breaks=0, ext_cnt_breaks=0, max_diffs=[], range_replaced=0,
                left=dict(qualified=0, failed_x=0, failed_y=0, end=None), right=dict(qualified=0, failed_x=0, failed_y=0, end=None),
                rs0_clamped=0, rs1_clamped=0, left_gap=None, right_gap=None, skipped=0, flagged_last=0, long_join_fills=0, refused=[])


def plan_hit(o, k, tlens, qlen, a, as_, cnt, mlen, split_inv):
    """one hit a[as_ : as_ + cnt] of the read's anchor list a (SEED_IGNORE marks are set in place) -> (hit dict, ev)"""
    ev = new_ev()
    n_a = len(a)
    rid, rev = (a[as_][0] << 1 & (1 << 64) - 1) >> 33, a[as_][0] >> 63
    tlen_all, kh = tlens[rid], k >> 1
    bw = int(o['bw'] * 1.5 + 1.)
    as1, cnt1 = fix_bad_ends(o, a, as_, cnt, mlen, ev)
    filter_bad_seeds(a, as1, cnt1, o['max_gap'] >> 1, ev)
    rs, qs = ax(a[as1]) - kh, ay(a[as1]) - kh
    re, qe = ax(a[as1 + cnt1 - 1]) - kh, ay(a[as1 + cnt1 - 1]) - kh
    # ---- the region the end extensions may reach
    rs0 = ax(a[as_]) + 1 - span(a[as_])
    qs0 = ay(a[as_]) + 1 - span(a[as_])
    if rs0 < 0:
        rs0 = 0
        ev['rs0_clamped'] = 1
    rs1 = qs1 = 0
    i, l = as_ - 1, 0
    ev['left']['end'] = 'index0'
    while i >= 0:
        if a[i][0] >> 32 != a[as_][0] >> 32:
            ev['left']['end'] = 'other'
            break
        x, y = ax(a[i]) + 1 - span(a[i]), ay(a[i]) + 1 - span(a[i])
        if x < rs0 and y < qs0:
            l += 1
            ev['left']['qualified'] += 1
            if l > o['min_cnt']:
                l = max(rs0 - x, qs0 - y)
                rs1, qs1 = rs0 - l, qs0 - l
                if rs1 < 0:
                    rs1 = 0
                    ev['rs1_clamped'] = 1
                ev['left']['end'] = 'found'
                break
        else:
            ev['left']['failed_x' if not x < rs0 else 'failed_y'] += 1
        i -= 1
    if qs > 0 and rs > 0:
        l = min(qs, o['max_gap'])
        ev['left_gap'] = dict(capped=qs > o['max_gap'], grown=l * o['a'] > o['q'], target_closer=rs < qs)
        qs1 = max(qs1, qs - l)
        qs0 = min(qs0, qs1)
        l += cdiv(l * o['a'] - o['q'], o['e']) if l * o['a'] > o['q'] else 0
        l = min(l, o['max_gap'])
        l = min(l, rs)
        rs1 = max(rs1, rs - l)
        rs0 = min(rs0, rs1)
        rs0 = min(rs0, rs)
    else:
        rs0, qs0 = rs, qs
    re0 = ax(a[as_ + cnt - 1]) + 1
    qe0 = ay(a[as_ + cnt - 1]) + 1
    re1, qe1 = tlen_all, qlen
    i, l = as_ + cnt, 0
    ev['right']['end'] = 'last'
    while i < n_a:
        if a[i][0] >> 32 != a[as_][0] >> 32:
            ev['right']['end'] = 'other'
            break
        x, y = ax(a[i]) + 1, ay(a[i]) + 1
        if x > re0 and y > qe0:
            l += 1
            ev['right']['qualified'] += 1
            if l > o['min_cnt']:
                l = max(x - re0, y - qe0)
                re1, qe1 = re0 + l, qe0 + l
                ev['right']['end'] = 'found'
                break
        else:
            ev['right']['failed_x' if not x > re0 else 'failed_y'] += 1
        i += 1
    if qe < qlen and re < tlen_all:
        l = min(qlen - qe, o['max_gap'])
        ev['right_gap'] = dict(capped=qlen - qe > o['max_gap'], grown=l * o['a'] > o['q'], target_closer=tlen_all - re < qlen - qe)
        qe1 = min(qe1, qe + l)
        qe0 = max(qe0, qe1)
        l += cdiv(l * o['a'] - o['q'], o['e']) if l * o['a'] > o['q'] else 0
        l = min(l, o['max_gap'])
        l = min(l, tlen_all - re)
        re1 = min(re1, re + l)
        re0 = max(re0, re1)
    else:
        re0, qe0 = re, qe
    hit = dict(as1=as1, cnt1=cnt1, qs=qs, rs=rs, qs0=qs0, qe0=qe0, rid=rid, rev=rev)
    # ---- the windows
    wins = []

    def window(kind, wqs, wql, wts, wtl, reversed_, w, zdrop, end_bonus, flag, anchor):
        refused = o['max_sw_mat'] > 0 and wtl * wql > o['max_sw_mat']
        raw = dict(qs=wqs, qlen=wql, ts=wts, tlen=wtl, reversed=reversed_, w=w, zdrop=zdrop, end_bonus=end_bonus, flag=flag, anchor=anchor,
                   refused=int(refused))
        if refused:
            ev['refused'].append(kind)
            wql = wtl = w = zdrop = end_bonus = 0
            flag |= EZ_REFUSED
        wins.append(dict(rid=rid, rev=rev, qs=wqs, qlen=wql, ts=wts, tlen=wtl, reversed=reversed_, w=w, zdrop=zdrop, end_bonus=end_bonus,
                         flag=flag, anchor=anchor, kind=kind, raw=raw))

    if qs > 0 and rs > 0:
        window('left', qs0, qs - qs0, rs0, rs - rs0, 1, bw, o['zdrop_inv'] if split_inv else o['zdrop'], o['end_bonus'],
               EZ_EXTZ_ONLY | EZ_RIGHT | EZ_REV_CIGAR, -1)
    for i in range(1, cnt1):
        fl = a[as1 + i][1]
        if fl & (SEED_IGNORE | SEED_TANDEM):
            if i != cnt1 - 1:
                ev['skipped'] += 1
                continue
            ev['flagged_last'] += 1
        re, qe = ax(a[as1 + i]) - kh, ay(a[as1 + i]) - kh
        if i == cnt1 - 1 or fl & SEED_LONG_JOIN or (qe - qs >= o['min_ksw_len'] and re - rs >= o['min_ksw_len']):
            bw1 = bw
            if fl & SEED_LONG_JOIN:
                bw1 = max(qe - qs, re - rs)
                ev['long_join_fills'] += 1
            window('fill', qs, qe - qs, rs, re - rs, 0, bw1, o['zdrop'], -1, EZ_APPROX_MAX, i)
            rs, qs = re, qe
    if qe < qe0 and re < re0:
        window('right', qe, qe0 - qe, re, re0 - re, 0, bw, o['zdrop'], o['end_bonus'], EZ_EXTZ_ONLY, -1)
    hit.update(qe=qe, re=re, re0=re0, rs0=rs0, n_jobs=len(wins), windows=wins)
    return hit, ev


def plan_ref(k, tlens, qlen, anchors, hits, **opt):
    """one read: anchors [(x, y)] (its squeezed list), hits [(as, cnt, mlen, split_inv)] in any order -> (hit dicts in that order, each
    with its `windows`; the anchors as planning leaves them [(x, y)]; ev per hit)"""
    o = dict(DEFAULTS)
    o.update(opt)
    a = [[int(x), int(y)] for x, y in anchors]
    out, evs = [], []
    for as_, cnt, mlen, split_inv in hits:
        h, ev = plan_hit(o, k, tlens, qlen, a, as_, cnt, mlen, split_inv)
        out.append(h)
        evs.append(ev)
    return out, [(x, y) for x, y in a], evs
