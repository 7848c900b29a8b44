"""Plain sequential restatement of the hit stage (csrc/hit_kernels.h and gen_regs .. join_long of csrc/hit_host.cpp): minimap2's
mm_gen_regs, mm_set_parent, mm_select_sub, mm_squeeze_a and mm_join_long on one read's chains, in Python integers, with numpy
float32 wherever the C code computes in `float`.  test_hit_ref.py pins it to the oracle's own functions (mmo_hits_from_chains);
test_hit_select_gpu.py compares the kernel and the host path with it, test_hit_host.py the host path alone on the CPU.

Input as the oracle takes it: u[c] = score << 32 | cnt and the chains' anchors (x, y) back to back, chains in the order of their
first anchors.  hit_ref() also returns what happened on the way (`ev`), so that the tests can assert that their cases reach the
mechanisms they were written for."""
import numpy as np

f32 = np.float32
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
SEED_LONG_JOIN = 1 << 40
KEYS = ('fx', 'fy', 'lx', 'ly', 'score', 'score0', 'cnt', 'as', 'parent', 'subsc', 'n_sub', 'mlen', 'blen', 'hash', 'sam_pri')
REFUSALS = ('adjacency', 'rid_strand', 'step', 'max_join_long', 'max_join_short', 'sc_thres', 'flank0', 'flank1')
DEFAULTS = dict(mask_level=0.5, pri_ratio=0.8, best_n=5, max_join_long=20000, max_join_short=2000, min_join_flank_sc=1000,
                min_join_flank_ratio=0.5, min_cnt=3, seed=11)


def hash64(key):
    key = (~key + (key << 21)) & M64
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & M64
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & M64
    key = key ^ key >> 28
    key = (key + (key << 31)) & M64
    return key


def wang32(key):
    key = (key + (~(key << 15) & M32)) & M32
    key ^= key >> 10
    key = (key + (key << 3)) & M32
    key ^= key >> 6
    key = (key + (~(key << 11) & M32)) & M32
    key ^= key >> 16
    return key


def x31_hash(s):
    b = s.encode() if isinstance(s, str) else bytes(s)
    if not b:
        return 0
    h = b[0]
    for c in b[1:]:
        h = ((h << 5) - h + c) & M32
    return h


def read_hash(name, qlen, seed):
    h = x31_hash(name) if name is not None else 0
    h ^= (wang32(qlen & M32) + wang32(seed)) & M32
    return wang32(h)


def i32(v):
    """the low 32 bits of v as a signed int: (int32_t)v"""
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def span_of(y):
    return y >> 32 & 0xff


def fuzzy_len(a, s, cnt):
    """mm_cal_fuzzy_len over anchors a[s : s + cnt] -> (mlen, blen)"""
    if cnt <= 0:
        return 0, 0
    mlen = blen = span_of(a[s][1])
    for i in range(s + 1, s + cnt):
        sp = span_of(a[i][1])
        tl = i32(a[i][0]) - i32(a[i - 1][0])
        ql = i32(a[i][1]) - i32(a[i - 1][1])
        blen += tl if tl > ql else ql
        mlen += sp if (tl > sp and ql > sp) else (tl if tl < ql else ql)
    return mlen, blen


def set_coor(r, qlen, a, ev=None):
    k, cnt = r['as'], r['cnt']
    fx, fy = a[k]
    lx, ly = a[k + cnt - 1]
    sp = span_of(fy)
    r['fx'], r['fy'], r['lx'], r['ly'] = fx, fy, lx, ly
    r['rev'] = fx >> 63
    r['rid'] = (fx << 1 & M64) >> 33
    if i32(fx) + 1 > sp:
        r['rs'] = i32(fx) + 1 - sp
    else:
        r['rs'] = 0
        if ev is not None and i32(fx) + 1 < sp:
            ev['rs_clamped'] += 1
    r['re'] = i32(lx) + 1
    if not r['rev']:
        r['qs'], r['qe'] = i32(fy) + 1 - sp, i32(ly) + 1
    else:
        r['qs'], r['qe'] = qlen - (i32(ly) + 1), qlen - (i32(fy) + 1 - sp)
    r['mlen'], r['blen'] = fuzzy_len(a, k, cnt)


def set_sam_pri(regs):
    n_pri = 0
    for r in regs:
        if r['id'] == r['parent']:
            n_pri += 1
            r['sam_pri'] = int(n_pri == 1)
        else:
            r['sam_pri'] = 0


def sync_regs(regs, ev):
    if not regs:
        return
    max_id = max(r['id'] for r in regs)
    tmp = [-1] * (max_id + 1 if max_id >= 0 else 1)
    for i, r in enumerate(regs):
        if r['id'] >= 0:
            tmp[r['id']] = i
    for i, r in enumerate(regs):
        r['id'] = i
        if r['parent'] == -2:
            r['parent'] = i
        elif 0 <= r['parent'] <= max_id and tmp[r['parent']] >= 0:
            r['parent'] = tmp[r['parent']]
        else:
            r['parent'] = -1
    set_sam_pri(regs)
    ev['resynced'] += 1


def same_coor(p, q):
    return p['qs'] == q['qs'] and p['qe'] == q['qe'] and p['rid'] == q['rid'] and p['rs'] == q['rs'] and p['re'] == q['re']


def new_events():
    ev = dict(kept_2nd=0, drop_ratio=0, drop_best_n=0, drop_identical=0, aliased_parent=0, joins=0, chained_joins=0,
              dropped_by_min_cnt=0, resynced=0, rs_clamped=0, hash_ties=0, multi_cover=0, triple_cover=0, n_sub_counted=0, n_sub_skipped=0,
              masked=0, mask_refused=0, by_ratio_only=0, by_diff_only=0)
    ev['join_refused_by'] = {k: 0 for k in REFUSALS}
    return ev


def hit_ref(k, name, qlen, u, a, **opt):
    """-> (hits: list of dicts with KEYS and qs, qe, rs, re, rid, rev; squeezed anchors: list of (x, y); ev)"""
    o = dict(DEFAULTS)
    o.update(opt)
    a = [(int(x), int(y)) for x, y in a]
    u = [int(v) for v in u]
    ev = new_events()
    n = len(u)
    if n == 0:
        return [], [], ev
    hash_ = read_hash(name, qlen, o['seed'])
    min_diff = 2 * k
    # ---- mm_gen_regs
    z, pos = [], 0
    for c in range(n):
        h = hash64((hash64(a[pos][0]) + hash64(a[pos][1]) & M64) ^ hash_) & M32
        cnt = i32(u[c])
        z.append((u[c] ^ h, pos << 32 | cnt & M32))
        pos += cnt
    assert pos == len(a)
    z.sort()
    regs = []
    for i in range(n):
        x, y = z[n - 1 - i]
        r = dict(id=i, parent=-1, score=i32(x >> 32), score0=i32(x >> 32), hash=x & M32, cnt=i32(y), subsc=0, n_sub=0, sam_pri=0)
        r['as'] = y >> 32
        set_coor(r, qlen, a, ev)
        regs.append(r)
    ev['hash_ties'] = sum(1 for i in range(1, n) if regs[i]['score'] == regs[i - 1]['score'])
    # ---- mm_set_parent (no hit has a base-level alignment yet)
    mask_level = f32(o['mask_level'])
    w = [0]
    regs[0]['parent'] = 0
    for i in range(1, n):
        ri = regs[i]
        si, ei = ri['qs'], ri['qe']
        cov = []
        for j in w:
            sj, ej = regs[j]['qs'], regs[j]['qe']
            if ej <= si or sj >= ei:
                continue
            cov.append((max(sj, si), min(ej, ei)))
        done = False
        if cov:
            cov.sort()
            x, uncov = si, 0
            for s, e in cov:
                if s > x:
                    uncov += s - x
                x = e if e > x else x
            if ei > x:
                uncov += ei - x
            if len(cov) >= 2 and uncov > 0:
                ev['multi_cover'] += 1
            if len(cov) >= 3 and uncov > 0:
                ev['triple_cover'] += 1
            for j in w:
                rp = regs[j]
                sj, ej = rp['qs'], rp['qe']
                if ej <= si or sj >= ei:
                    continue
                mn, mx = min(ej - sj, ei - si), max(ej - sj, ei - si)
                if si < sj:
                    ol = 0 if ei < sj else (ei - sj if ei < ej else ej - sj)
                else:
                    ol = 0 if ej < si else (ej - si if ej < ei else ei - si)
                if f32(ol) / f32(mn) - f32(uncov) / f32(mx) > mask_level:
                    ri['parent'] = rp['parent']
                    rp['subsc'] = max(rp['subsc'], ri['score'])
                    if ri['cnt'] >= rp['cnt']:
                        rp['n_sub'] += 1
                        ev['n_sub_counted'] += 1
                    else:
                        ev['n_sub_skipped'] += 1
                    ev['masked'] += 1
                    done = True
                    break
                ev['mask_refused'] += 1
        if not done:
            w.append(i)
            ri['parent'] = i
            ri['n_sub'] = 0
    # ---- mm_select_sub, in place: r[p] is read as the compaction has left it
    pri_ratio = f32(o['pri_ratio'])
    if pri_ratio > 0:
        orig = list(regs)   # (no hit is changed in this loop: slot p holds the parent itself, or what was moved over it)
        n_2nd = kk = 0

        def verdict(ri, rp):
            by_ratio = bool(f32(ri['score']) >= f32(rp['score']) * pri_ratio)
            by_diff = ri['score'] + min_diff >= rp['score']
            if not (by_ratio or by_diff):
                return 'drop_ratio', by_ratio, by_diff
            if not n_2nd < o['best_n']:
                return 'drop_best_n', by_ratio, by_diff
            if same_coor(ri, rp):
                return 'drop_identical', by_ratio, by_diff
            return 'kept_2nd', by_ratio, by_diff
        for i in range(n):
            ri = regs[i]
            p = ri['parent']
            if p == i:
                regs[kk] = ri
                kk += 1
                continue
            v, by_ratio, by_diff = verdict(ri, regs[p])
            if regs[p] is not orig[p] and verdict(ri, orig[p])[0] != v:
                ev['aliased_parent'] += 1
            ev[v] += 1
            if by_ratio != by_diff:
                ev['by_ratio_only' if by_ratio else 'by_diff_only'] += 1
            if v == 'kept_2nd':
                regs[kk] = ri
                kk += 1
                n_2nd += 1
        if kk != n:
            regs = regs[:kk]
            sync_regs(regs, ev)
    # ---- mm_squeeze_a
    order = sorted(range(len(regs)), key=lambda i: (regs[i]['as'], i))
    sq = []
    for i in order:
        r = regs[i]
        s = r['as']
        r['as'] = len(sq)
        sq.extend(a[s:s + r['cnt']])
    n_a = len(sq)
    # ---- mm_join_long
    if len(regs) >= 2:
        aux = sorted((r['as'], i) for i, r in enumerate(regs) if r['parent'] == i or r['parent'] < 0)
        n_drop = 0
        refused = ev['join_refused_by']
        absorbed = set()
        for t in range(len(aux) - 1, 0, -1):
            r0, r1 = regs[aux[t - 1][1]], regs[aux[t][1]]
            if r0['as'] + r0['cnt'] != r1['as']:
                refused['adjacency'] += 1
                continue
            if r0['rid'] != r1['rid'] or r0['rev'] != r1['rev']:
                refused['rid_strand'] += 1
                continue
            a0x, a0y = sq[r0['as'] + r0['cnt'] - 1]
            a1x, a1y = sq[r1['as']]
            if a1x <= a0x or i32(a1y) <= i32(a0y):
                refused['step'] += 1
                continue
            max_gap = min_gap = i32(a1y) - i32(a0y)
            dx = a1x - a0x
            max_gap = max_gap if max_gap > dx else i32(dx)
            min_gap = min_gap if min_gap < dx else i32(dx)
            if max_gap > o['max_join_long']:
                refused['max_join_long'] += 1
                continue
            if min_gap > o['max_join_short']:
                refused['max_join_short'] += 1
                continue
            sc_thres = int(float(f32(o['min_join_flank_sc']) / f32(o['max_join_long']) * f32(max_gap)) + .499)
            if r0['score'] < sc_thres or r1['score'] < sc_thres:
                refused['sc_thres'] += 1
                continue
            min_flank_len = int(f32(max_gap) * f32(o['min_join_flank_ratio']))
            if r0['re'] - r0['rs'] < min_flank_len or r0['qe'] - r0['qs'] < min_flank_len:
                refused['flank0'] += 1
                continue
            if r1['re'] - r1['rs'] < min_flank_len or r1['qe'] - r1['qs'] < min_flank_len:
                refused['flank1'] += 1
                continue
            sq[r1['as']] = (a1x, a1y | SEED_LONG_JOIN)
            r0['cnt'] += r1['cnt']
            r0['score'] += r1['score']
            set_coor(r0, qlen, sq)
            r1['cnt'] = 0
            r1['parent'] = r0['id']
            n_drop += 1
            ev['joins'] += 1
            if r1['id'] in absorbed:
                ev['chained_joins'] += 1
            absorbed.add(r0['id'])
        if n_drop > 0:
            for r in regs:
                if r['parent'] >= 0 and r['id'] != r['parent']:
                    pp = regs[r['parent']]['parent']
                    if pp >= 0 and pp != r['parent']:
                        r['parent'] = pp
            ev['dropped_by_min_cnt'] += sum(1 for r in regs if 0 < r['cnt'] < o['min_cnt'])
            regs = [r for r in regs if not r['cnt'] < o['min_cnt']]
            sync_regs(regs, ev)
    assert len(sq) == n_a
    return regs, sq, ev
