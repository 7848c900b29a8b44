"""A plain restatement of the chaining stage (oracle/mm2_oracle.c mmo_chain: the chain DP with its skip counter and iteration cut, the
chain ends walked back to their peaks, their descending sort, the ordered backtrack with the "taken" marks, the chains reordered by
their first anchor) plus mm_cal_fuzzy_len per chain, with a RECORD of the mechanisms a case reached.  test_chain_ref.py pins it to
the oracle; test_chain_stage_gpu.py compares the GPU kernels with it.  Sequential, integers only, except the gap cost: the average
seed length is a float32 quotient as in the oracle, the cost is computed in double from it."""
import numpy as np

OPT_KEYS = ('max_gap', 'bw', 'max_chain_skip', 'max_chain_iter', 'min_cnt', 'min_chain_score')
DEFAULTS = dict(max_gap=5000, bw=500, max_chain_skip=25, max_chain_iter=5000, min_cnt=3, min_chain_score=40)
COUNTERS = ('skip_break', 'skip_dec', 'iter_cut', 'far128', 'far_tile', 'peak_back', 'branch', 'stop_taken', 'sub_reject', 'cnt_reject',
            'discarded_taken_hit', 'n_ends')
REC_KEYS = ('fx', 'fy', 'lx', 'ly', 'mlen', 'blen')


def options(**kw):
    o = dict(DEFAULTS)
    assert set(kw) <= set(OPT_KEYS), kw
    o.update(kw)
    return o


def _i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


def fuzzy_len(chain):
    """mm_cal_fuzzy_len on the anchors [(x, y), ...] of one chain -> (mlen, blen)"""
    ml = bl = chain[0][1] >> 32 & 0xff
    for (px, py), (x, y) in zip(chain, chain[1:]):
        span = y >> 32 & 0xff
        tl, ql = _i32(x) - _i32(px), _i32(y) - _i32(py)
        bl += tl if tl > ql else ql
        ml += span if tl > span and ql > span else (tl if tl < ql else ql)
    return ml, bl


def chain_ref(opt, a):
    """opt: dict of OPT_KEYS; a: the read's anchors, uint64 [n, 2], sorted -> (u list of score << 32 | cnt, b uint64 [n_chained, 2],
    recs list of REC_KEYS tuples, record dict of COUNTERS), chains in the order of their first anchors"""
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 2)
    n = len(a)
    rec = dict.fromkeys(COUNTERS, 0)
    empty = ([], np.zeros((0, 2), dtype=np.uint64), [], rec)
    if n == 0:
        return empty
    max_dist, bw, max_skip = opt['max_gap'], opt['bw'], opt['max_chain_skip']
    max_iter, min_cnt, min_sc = opt['max_chain_iter'], opt['min_cnt'], opt['min_chain_score']
    X = [int(v) for v in a[:, 0]]
    Y = [int(v) for v in a[:, 1]]
    Q = [_i32(y) for y in Y]
    S = [y >> 32 & 0xff for y in Y]
    avg = float(np.float32(sum(S)) / np.float32(n))      # (float)sum / n
    f, p, t, v = [0] * n, [-1] * n, [0] * n, [0] * n
    st = 0
    for i in range(n):
        ri, qi, q_span = X[i], Q[i], S[i]
        max_f, max_j, n_skip = q_span, -1, 0
        while st < i and ri > X[st] + max_dist:
            st += 1
        if i - st > max_iter:
            st = i - max_iter
            rec['iter_cut'] += 1
        past = 0
        for j in range(i - 1, st - 1, -1):
            if i - j > 64:
                past = 1                             # (visited: the walk was not broken inside the first 64)
            dr, dq = ri - X[j], qi - Q[j]
            if dr == 0 or dq <= 0 or dq > max_dist:
                continue
            dd = dr - dq if dr > dq else dq - dr
            if dd > bw:
                continue
            if i - j > 128:
                rec['far128'] += 1
            min_d = dq if dq < dr else dr
            sc = q_span if min_d > q_span else min_d
            log_dd = dd.bit_length() - 1 if dd else 0
            sc -= int(dd * .01 * avg) + (log_dd >> 1)
            sc += f[j]
            if sc > max_f:
                max_f, max_j = sc, j
                if n_skip > 0:
                    n_skip -= 1
                    rec['skip_dec'] += 1
            elif t[j] == i + 1:                      # (marks are i + 1, so that 0 means "never marked")
                n_skip += 1
                if n_skip > max_skip:
                    rec['skip_break'] += 1
                    break
            if p[j] >= 0:
                t[p[j]] = i + 1
        rec['far_tile'] += past
        f[i], p[i] = max_f, max_j
        v[i] = v[max_j] if max_j >= 0 and v[max_j] > max_f else max_f
    # chain ends: anchors nobody points to, walked back to their peak
    kids = [0] * n
    for i in range(n):
        if p[i] >= 0:
            kids[p[i]] += 1
    rec['branch'] = sum(1 for k in kids if k >= 2)
    ends = []
    for i in range(n):
        if kids[i] == 0 and v[i] >= min_sc:
            j = i
            while j >= 0 and f[j] < v[j]:
                j = p[j]
            if j < 0:
                j = i
            if j != i:
                rec['peak_back'] += 1
            ends.append(f[j] << 32 | j)
    rec['n_ends'] = len(ends)
    ends.sort(reverse=True)
    # backtrack, best end first; an anchor belongs to one chain only, and stays taken when its end is discarded
    taken = [-1] * n         # the rank of the end that took the anchor
    kept = [False] * len(ends)
    chains = []
    for e, ue in enumerate(ends):
        j, sc, walk = ue & 0xffffffff, ue >> 32, []
        while True:
            walk.append(j)
            taken[j] = e
            j = p[j]
            if not (j >= 0 and taken[j] < 0):
                break
        ok = True
        if j >= 0:
            rec['stop_taken'] += 1
            if not kept[taken[j]]:
                rec['discarded_taken_hit'] += 1
            sc -= f[j]
            if sc < min_sc:
                ok = False
                rec['sub_reject'] += 1
        if ok and len(walk) < min_cnt:
            ok = False
            rec['cnt_reject'] += 1
        if ok:
            kept[e] = True
            chains.append((sc, walk[::-1]))
    if not chains:
        return empty
    # chains by the reference coordinate of their first anchor, then by their place in the backtrack's order
    order, k = [], 0
    for c, (sc, idx) in enumerate(chains):
        order.append((X[idx[0]], k << 32 | c, c))
        k += len(idx)
    order.sort()
    u, rows, recs = [], [], []
    for _, _, c in order:
        sc, idx = chains[c]
        u.append(sc << 32 | len(idx))
        rows.extend(idx)
        ch = [(X[i], Y[i]) for i in idx]
        recs.append((ch[0][0], ch[0][1], ch[-1][0], ch[-1][1]) + fuzzy_len(ch))
    return u, a[rows].copy(), recs, rec
