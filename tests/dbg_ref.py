"""A plain restatement of the reference's de Bruijn graph consensus (realign/debruijn_graph.cpp), written from its source text
with dicts and lists, as the yardstick for the host build and the kernel of csrc/dbg_core.h.  The reference's own library needs
Boost, which is not to be had here, so there is no golden of its output: tests/test_dbg_ref.py pins this file by cases derived by
hand from the source.

    get_consensus(ref, reads, bad)  ->  (sorted haplotypes, k used or 0)

ref and the reads are str; bad holds, per read, the set (any iterable) of its low-quality positions.  order_matters(...) tells
whether the cap of 256 paths was passed by the very last pop -- the one place where the reference's answer depends on the order
of its adjacency lists (pointer order there, ascending k-mer order here).
"""
from collections import deque

K_FIRST, K_LAST, PATH_LIMIT = 10, 101, 256


def k_bounds(ref):   # KMinMaxFromReference
    max_k = min(K_LAST, len(ref) - 1)
    for k in range(K_FIRST, max_k + 1):
        kmers = [ref[i:i + k] for i in range(len(ref) - k + 1)]
        if len(set(kmers)) == len(kmers):
            return k, max_k
    return None, max_k


def read_edges(read, bad, k):   # AddEdgesForRead + AddKmersAndEdges: (from k-mer, to k-mer) per traversal
    bad = set(bad)
    n = len(read)
    stop = n - k
    i = 0
    while i < stop:
        nxt = next((j for j in range(i, n) if read[j] not in 'ACGT' or j in bad), n)
        end = nxt - k
        if end > 0:
            for j in range(i + 1, end + 1):
                yield read[j - 1:j - 1 + k], read[j:j + k]
        i = nxt + 1


def build_graph(ref, reads, bad, k):
    """-> {from: {to: [weight, is_ref]}} with every vertex as a key"""
    g = {}

    def add(a, b, is_ref):
        g.setdefault(b, {})
        e = g.setdefault(a, {}).setdefault(b, [0, False])
        e[0] += 1
        e[1] = e[1] or is_ref
    for j in range(1, len(ref) - k + 1):
        add(ref[j - 1:j - 1 + k], ref[j:j + k], True)
    for r, b in zip(reads, bad):
        for a, c in read_edges(r, b, k):
            add(a, c, False)
    return g


def has_cycle(g):   # a depth-first search over every vertex that meets a back edge
    colour = dict.fromkeys(g, 0)
    for root in g:
        if colour[root]:
            continue
        colour[root] = 1
        stack = [(root, iter(g[root]))]
        while stack:
            v, it = stack[-1]
            for t in it:
                if colour[t] == 1:
                    return True
                if colour[t] == 0:
                    colour[t] = 1
                    stack.append((t, iter(g[t])))
                    break
            else:
                colour[v] = 2
                stack.pop()
    return False


def reach(adj, start):
    seen, todo = {start}, [start]
    while todo:
        for t in adj[todo.pop()]:
            if t not in seen:
                seen.add(t)
                todo.append(t)
    return seen


def prune(g, source, sink):
    kept = {a: sorted(b for b, (w, is_ref) in out.items() if is_ref or w >= 2) for a, out in g.items()}
    back = {a: [] for a in g}
    for a, out in kept.items():
        for b in out:
            back[b].append(a)
    alive = reach(kept, source) & reach(back, sink)
    return {a: [b for b in out if b in alive] for a, out in kept.items() if a in alive}


def candidate_paths(adj, source, sink):
    """-> (paths, whether the count passed the cap at the last pop only)"""
    done, queue = [], deque([[source]])
    over = False
    while queue:
        if len(done) + len(queue) > PATH_LIMIT:
            return [], False
        path = queue.popleft()
        for t in adj[path[-1]]:
            (done if t == sink or not adj[t] else queue).append(path + [t])
        over = len(done) + len(queue) > PATH_LIMIT
    return done, over


def consensus(ref, reads, bad):
    """-> (haplotypes, k, order_matters)"""
    min_k, max_k = k_bounds(ref)
    if min_k is None:
        return [], 0, False
    for k in range(min_k, max_k + 1):
        g = build_graph(ref, reads, bad, k)
        if has_cycle(g):
            continue
        source, sink = ref[:k], ref[len(ref) - k:]
        paths, over = candidate_paths(prune(g, source, sink), source, sink)
        return sorted(''.join(v[0] for v in p) + p[-1][1:] for p in paths), k, over
    return [], 0, False


def get_consensus(ref, reads, bad=None):
    bad = [()] * len(reads) if bad is None else bad
    haps, k, _ = consensus(ref, reads, bad)
    return haps, k


def order_matters(ref, reads, bad=None):
    return consensus(ref, reads, [()] * len(reads) if bad is None else bad)[2]
