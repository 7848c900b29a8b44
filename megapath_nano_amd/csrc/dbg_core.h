// The rules of the de Bruijn graph consensus (include/mpn_dbg.h), written once for the device and for the host.
//
// dbg_window() turns one window -- a reference, its reads and a byte-per-base bad mask -- into the sorted candidate haplotypes of
// the first k whose graph has no cycle.  It is written for `nl` lanes that meet at dbg_sync(): the kernel (dbg_kernels.hip) calls
// it with the 256 lanes of the workgroup that owns the window, scripts/dbg_host_check.cpp with one lane, where every barrier is
// nothing and every atomic a plain operation.  The two are the same text, so what the host check proves under the sanitizers
// (the rules, every index, every bound of a loop) is what the kernel runs; only the interleaving of the lanes is the device's own.
//
// The graph of one k lives in an open-addressing table of k-mers (vertices).  A vertex is the offset of one occurrence of its
// k-mer in the window's bases; equal hash values are resolved by comparing the k bases.  A successor of a k-mer is named by the
// base that follows it, so a vertex holds five successor slots -- A, C, G, T and `other` -- and as many predecessor slots, named by
// the base in front.  Reads contribute only A, C, G, T.  `other` is a reference byte outside ACGT (N, IUPAC): the reference's
// k-mers are distinct at every k that gets as far as its edges, so a vertex has at most one edge through such a byte each way.
// An edge's weight is the number of reads that walk it; `refmask` marks the reference's edges, whose weight nobody asks for.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DBG_FN __device__ inline
#else
#define DBG_FN static inline
#endif

enum {
    DBG_OK = 0,          // k found; the haplotypes of its graph (possibly none)
    DBG_NO_K = 1,        // no k in 10 .. max_k gives distinct reference k-mers and an acyclic graph: no haplotypes, k = 0
    DBG_PATH_CAP = 2,    // k found, but more than 256 paths were alive at a pop: no haplotypes
    DBG_TABLE_FULL = 3,  // the k-mer table is too small: nothing was truncated, the window wants a larger table
    DBG_HAP_FULL = 4,    // a path grew past the haplotype buffers: the window wants longer ones
    DBG_ARENA_FULL = 5,  // (kernel only) no room left for the window's strings in the pass's output
};

constexpr int DBG_K_FIRST = 10, DBG_K_LAST = 101;
constexpr int DBG_PATH_LIMIT = 256;              // CandidatePaths: terminated + queued paths above this at a pop end the walk
constexpr int DBG_MAXP = DBG_PATH_LIMIT + 8;     // paths that can exist: 256 before the last pop, which adds at most 4
constexpr uint32_t DBG_NONE = 0xffffffffu;
constexpr uint32_t DBG_MIN_SLOTS = 1024;         // the table refuses inserts at half full; <= 256 lanes can overshoot that by 255

// ---- what differs between the device and the host ----------------------------------------
#if defined(__HIPCC__)
DBG_FN void dbg_sync() { __syncthreads(); }
DBG_FN uint32_t dbg_add(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
DBG_FN uint32_t dbg_or(uint32_t *p, uint32_t v) { return atomicOr(p, v); }
DBG_FN uint32_t dbg_cas(uint32_t *p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
// words that other lanes change with atomics are read and written past the CU's L1
DBG_FN uint32_t dbg_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DBG_FN void dbg_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
DBG_FN void dbg_sync() {}
DBG_FN uint32_t dbg_add(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
DBG_FN uint32_t dbg_or(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o | v; return o; }
DBG_FN uint32_t dbg_cas(uint32_t *p, uint32_t expect, uint32_t v) { const uint32_t o = *p; if (o == expect) *p = v; return o; }
DBG_FN uint32_t dbg_load(const uint32_t *p) { return *p; }
DBG_FN void dbg_store(uint32_t *p, uint32_t v) { *p = v; }
#endif

// ---- one window's input, the workspace of the workgroup that owns it, and what the lanes share -----
struct DbgWindow {
    const uint8_t *seq;        // the reference's bytes, then the reads back to back: `total` bytes
    const uint8_t *mask;       // `total` bytes, nonzero where a read's base is bad (the reference's part is not read)
    const uint32_t *read_off;  // n_reads + 1 offsets into seq: read r is [read_off[r], read_off[r + 1]), read_off[0] == ref_len
    uint32_t ref_len, n_reads, total;
};

struct DbgWork {
    uint32_t slots;     // power of two, >= DBG_MIN_SLOTS
    uint32_t hap_cap;   // bytes of one haplotype buffer
    uint32_t *loc;      // [slots] offset of the vertex's k-mer in seq, DBG_NONE: empty
    uint32_t *succ;     // [5][slots]
    uint32_t *pred;     // [5][slots]
    uint32_t *w;        // [4][slots] reads over the edge to successor A, C, G, T
    uint32_t *refmask;  // [slots] bit c: the edge to successor c is the reference's
    uint32_t *indeg;    // [slots]
    uint32_t *flags;    // [slots] bit 0: reachable from the source, bit 1: reaches the sink (over the edges that pruning keeps)
    uint32_t *order;    // [slots] work lists of the peel and of the two reachability walks
    uint32_t *refslot;  // [ref_len] the vertex of each reference k-mer
    uint8_t *rem;       // [total] good bases from here to the end of the run, capped at 255
    uint8_t *hap;       // [DBG_MAXP][hap_cap]
};

struct DbgShared {      // LDS on the device
    uint32_t dup, full, nvert, tail;
    uint32_t cq[DBG_MAXP], ct[DBG_MAXP];            // per queued path: children that go on, children that end
    uint32_t pv[2][DBG_MAXP], pb[2][DBG_MAXP];      // the queue of this level and of the next: vertex, buffer
    uint32_t term_buf[DBG_MAXP], term_len[DBG_MAXP];
    uint32_t out_buf[DBG_MAXP], out_len[DBG_MAXP];  // the result: the haplotypes' buffers and lengths in sorted order
};

DBG_FN uint64_t dbg_work_words(uint32_t slots) { return (uint64_t)slots * 19; }   // the uint32 arrays that scale with the table

// every lane gets the value that *p has once all lanes have arrived, and nobody changes it before all have read it
DBG_FN uint32_t dbg_bcast(const uint32_t *p) {
    dbg_sync();
    const uint32_t v = *(const volatile uint32_t *)p;
    dbg_sync();
    return v;
}

DBG_FN int dbg_idx(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4; }

DBG_FN uint32_t dbg_hash(const uint8_t *s, int k) {
    uint32_t h = 2166136261u;
    for (int i = 0; i < k; ++i) h = (h ^ s[i]) * 16777619u;
    h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12;
    return h;
}

DBG_FN bool dbg_same(const uint8_t *a, const uint8_t *b, int k) {
    for (int i = 0; i < k; ++i) if (a[i] != b[i]) return false;
    return true;
}

// The vertex of the k-mer at seq[p .. p + k): found, or claimed.  DBG_NONE with sh->full set when the table is half full.
DBG_FN uint32_t dbg_vertex(const DbgWindow &win, const DbgWork &wk, DbgShared *sh, int k, uint32_t p, bool *existed) {
    const uint32_t m = wk.slots - 1;
    uint32_t s = dbg_hash(win.seq + p, k) & m;
    for (uint32_t probe = 0; probe < wk.slots; ++probe, s = (s + 1) & m) {
        uint32_t cur = dbg_load(&wk.loc[s]);
        if (cur == DBG_NONE) {
            if (dbg_load(&sh->nvert) >= wk.slots / 2) break;
            cur = dbg_cas(&wk.loc[s], DBG_NONE, p);
            if (cur == DBG_NONE) { dbg_add(&sh->nvert, 1); *existed = false; return s; }
        }
        if (cur == p || dbg_same(win.seq + cur, win.seq + p, k)) { *existed = true; return s; }
    }
    dbg_store(&sh->full, 1);
    return DBG_NONE;
}

// Is there an edge from v to its successor c: at all (the cycle test), or after pruning (reference edge, or two reads)
DBG_FN bool dbg_edge(const DbgWork &wk, uint32_t v, int c, bool pruned) {
    if ((dbg_load(&wk.refmask[v]) >> c) & 1) return true;
    return c < 4 && dbg_load(&wk.w[(uint32_t)c * wk.slots + v]) >= (pruned ? 2u : 1u);
}

// Work-list rounds over wk.order: the entries [head, tail) are expanded, what that appends is the next round.  The three uses
// differ in what expanding a vertex means.  Rounds are bounded by the number of vertices: every round appends one at least, and a
// vertex is appended once.  -> the number of vertices that went through the list
enum { DBG_PEEL, DBG_FWD, DBG_BWD };
DBG_FN uint32_t dbg_rounds(const DbgWindow &win, const DbgWork &wk, DbgShared *sh, int k, int mode, int lane, int nl) {
    uint32_t head = 0;
    for (;;) {
        const uint32_t tail = dbg_bcast(&sh->tail);
        if (head == tail) return tail;
        for (uint32_t i = head + lane; i < tail; i += nl) {
            const uint32_t v = wk.order[i];
            if (mode == DBG_BWD) {
                // v's last base names the edge at each of its predecessors
                const int c = dbg_idx(win.seq[dbg_load(&wk.loc[v]) + k - 1]);
                for (int pi = 0; pi < 5; ++pi) {
                    const uint32_t a = dbg_load(&wk.pred[(uint32_t)pi * wk.slots + v]);
                    if (a == DBG_NONE || !dbg_edge(wk, a, c, true)) continue;
                    if (!(dbg_or(&wk.flags[a], 2) & 2)) wk.order[dbg_add(&sh->tail, 1)] = a;
                }
                continue;
            }
            for (int c = 0; c < 5; ++c) {
                if (!dbg_edge(wk, v, c, mode == DBG_FWD)) continue;
                const uint32_t t = dbg_load(&wk.succ[(uint32_t)c * wk.slots + v]);
                if (mode == DBG_PEEL) {
                    if (dbg_add(&wk.indeg[t], 0xffffffffu) == 1) wk.order[dbg_add(&sh->tail, 1)] = t;
                } else if (!(dbg_or(&wk.flags[t], 1) & 1)) {
                    wk.order[dbg_add(&sh->tail, 1)] = t;
                }
            }
        }
        head = tail;
    }
}

// The successors of v that pruning keeps, in ascending order of their k-mers (that is, of the base that names them).
DBG_FN int dbg_children(const DbgWindow &win, const DbgWork &wk, int k, uint32_t v, uint32_t *child, uint8_t *base) {
    int n = 0;
    for (int c = 0; c < 5; ++c) {
        if (!dbg_edge(wk, v, c, true)) continue;
        const uint32_t t = dbg_load(&wk.succ[(uint32_t)c * wk.slots + v]);
        if ((dbg_load(&wk.flags[t]) & 3) != 3) continue;
        const uint8_t b = c < 4 ? (uint8_t)"ACGT"[c] : win.seq[dbg_load(&wk.loc[t]) + k - 1];
        int at = n++;
        for (; at > 0 && base[at - 1] > b; --at) { base[at] = base[at - 1]; child[at] = child[at - 1]; }
        base[at] = b;
        child[at] = t;
    }
    return n;
}

DBG_FN bool dbg_less(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb) {   // std::string's operator<
    const uint32_t n = la < lb ? la : lb;
    for (uint32_t i = 0; i < n; ++i) if (a[i] != b[i]) return a[i] < b[i];
    return la < lb;
}

// -> status (the same in every lane); *k_out the k used or 0; *n_out haplotypes, described by sh->out_buf / sh->out_len
DBG_FN int dbg_window(const DbgWindow &win, const DbgWork &wk, DbgShared *sh, int lane, int nl, int *k_out, int *n_out) {
    *k_out = 0;
    *n_out = 0;
    const uint32_t S = wk.slots, L = win.ref_len;
    const int max_k = (int)L - 1 < DBG_K_LAST ? (int)L - 1 : DBG_K_LAST;      // KMinMaxFromReference
    if (max_k < DBG_K_FIRST) return DBG_NO_K;
    // good bases from each base of a read to the end of its run: an edge at p needs k + 1 of them, at every k
    for (uint32_t r = lane; r < win.n_reads; r += nl) {
        uint32_t run = 0;
        for (uint32_t p = win.read_off[r + 1]; p-- > win.read_off[r];) {
            const bool good = dbg_idx(win.seq[p]) < 4 && !win.mask[p];
            run = good ? (run < 255 ? run + 1 : 255) : 0;
            wk.rem[p] = (uint8_t)run;
        }
    }
    for (int k = DBG_K_FIRST; k <= max_k; ++k) {
        for (uint32_t s = lane; s < S; s += nl) {
            wk.loc[s] = DBG_NONE;
            for (int c = 0; c < 5; ++c) { wk.succ[c * S + s] = DBG_NONE; wk.pred[c * S + s] = DBG_NONE; }
            for (int c = 0; c < 4; ++c) wk.w[c * S + s] = 0;
            wk.refmask[s] = 0; wk.indeg[s] = 0; wk.flags[s] = 0;
        }
        if (lane == 0) { sh->dup = 0; sh->full = 0; sh->nvert = 0; sh->tail = 0; }
        dbg_sync();
        // the reference's k-mers: one that is there already is a repeat, and a repeat is a cycle (and k is below min_k)
        const uint32_t n_ref = L - k + 1;
        for (uint32_t p = lane; p < n_ref; p += nl) {
            bool existed = false;
            wk.refslot[p] = dbg_vertex(win, wk, sh, k, p, &existed);
            if (existed) dbg_store(&sh->dup, 1);
        }
        if (dbg_bcast(&sh->full)) return DBG_TABLE_FULL;
        if (dbg_bcast(&sh->dup)) continue;
        // edges: the reference's, and one per run of k + 1 good bases of a read
        for (uint32_t p = lane; p + 1 < n_ref; p += nl) {
            const uint32_t a = wk.refslot[p], b = wk.refslot[p + 1];
            const int c = dbg_idx(win.seq[p + k]);
            dbg_store(&wk.succ[c * S + a], b);
            dbg_store(&wk.refmask[a], 1u << c);
            dbg_store(&wk.pred[dbg_idx(win.seq[p]) * S + b], a);
        }
        for (uint32_t p = L + lane; p < win.total; p += nl) {
            if (wk.rem[p] < k + 1) continue;
            if (dbg_load(&sh->full)) break;
            bool e = false;
            const uint32_t a = dbg_vertex(win, wk, sh, k, p, &e);
            const uint32_t b = a == DBG_NONE ? DBG_NONE : dbg_vertex(win, wk, sh, k, p + 1, &e);
            if (b == DBG_NONE) break;
            const int c = dbg_idx(win.seq[p + k]);
            dbg_add(&wk.w[c * S + a], 1);
            dbg_store(&wk.succ[c * S + a], b);
            dbg_store(&wk.pred[dbg_idx(win.seq[p]) * S + b], a);
        }
        if (dbg_bcast(&sh->full)) return DBG_TABLE_FULL;
        const uint32_t nvert = dbg_bcast(&sh->nvert);
        // HasCycle, on the whole graph: peel off the vertices nobody points to until nothing changes
        for (uint32_t s = lane; s < S; s += nl) {
            if (dbg_load(&wk.loc[s]) == DBG_NONE) continue;
            for (int c = 0; c < 5; ++c)
                if (dbg_edge(wk, s, c, false)) dbg_add(&wk.indeg[dbg_load(&wk.succ[c * S + s])], 1);
        }
        dbg_sync();
        for (uint32_t s = lane; s < S; s += nl)
            if (dbg_load(&wk.loc[s]) != DBG_NONE && dbg_load(&wk.indeg[s]) == 0) wk.order[dbg_add(&sh->tail, 1)] = s;
        if (dbg_rounds(win, wk, sh, k, DBG_PEEL, lane, nl) != nvert) continue;
        // Prune: what the source reaches and what reaches the sink, over reference edges and edges of weight >= 2
        *k_out = k;
        const uint32_t source = wk.refslot[0], sink = wk.refslot[n_ref - 1];
        if (lane == 0) { wk.order[0] = source; dbg_or(&wk.flags[source], 1); sh->tail = 1; }
        dbg_rounds(win, wk, sh, k, DBG_FWD, lane, nl);
        if (lane == 0) { wk.order[0] = sink; dbg_or(&wk.flags[sink], 2); sh->tail = 1; }
        dbg_rounds(win, wk, sh, k, DBG_BWD, lane, nl);
        // CandidatePaths, a level of the queue at a time.  Every path of a level has k + level bases in its buffer.
        uint32_t nq = 1, nt = 0, nbuf = 1, len = (uint32_t)k, cur = 0;
        if (len + 1 > wk.hap_cap) return DBG_HAP_FULL;
        for (uint32_t i = lane; i < len; i += nl) wk.hap[i] = win.seq[i];
        if (lane == 0) { sh->pv[0][0] = source; sh->pb[0][0] = 0; }
        dbg_sync();
        while (nq > 0) {
            if (len + 1 > wk.hap_cap) return DBG_HAP_FULL;
            uint32_t child[5];
            uint8_t base[5];
            for (uint32_t i = lane; i < nq; i += nl) {
                const int n = dbg_children(win, wk, k, sh->pv[cur][i], child, base);
                uint32_t t = 0;
                for (int j = 0; j < n; ++j) t += child[j] == sink;
                sh->cq[i] = (uint32_t)n - t;
                sh->ct[i] = t;
            }
            dbg_sync();
            // the count before the level's last pop is the largest any pop of it sees (a path that is popped has a child)
            uint32_t sum_q = 0, sum_t = 0, before_last = nt + nq;
            for (uint32_t i = 0; i < nq; ++i) {
                if (i + 1 == nq) before_last = nt + nq + sum_q + sum_t - i;
                sum_q += sh->cq[i];
                sum_t += sh->ct[i];
            }
            if (before_last > (uint32_t)DBG_PATH_LIMIT || sum_q + sum_t < nq) { *n_out = 0; return DBG_PATH_CAP; }
            for (uint32_t i = lane; i < nq; i += nl) {
                uint32_t qpos = 0, tpos = nt, bpos = nbuf;
                for (uint32_t j = 0; j < i; ++j) { qpos += sh->cq[j]; tpos += sh->ct[j]; bpos += sh->cq[j] + sh->ct[j] - 1; }
                const int n = dbg_children(win, wk, k, sh->pv[cur][i], child, base);
                const uint32_t own = sh->pb[cur][i];
                for (int j = 0; j < n; ++j) {
                    const uint32_t buf = j == 0 ? own : bpos++;
                    uint8_t *dst = wk.hap + (uint64_t)buf * wk.hap_cap;
                    if (j > 0) {
                        const uint8_t *src = wk.hap + (uint64_t)own * wk.hap_cap;
                        for (uint32_t b = 0; b < len; ++b) dst[b] = src[b];
                    }
                    dst[len] = base[j];
                    if (child[j] == sink) { sh->term_buf[tpos] = buf; sh->term_len[tpos] = len + 1; ++tpos; }
                    else { sh->pv[cur ^ 1][qpos] = child[j]; sh->pb[cur ^ 1][qpos] = buf; ++qpos; }
                }
            }
            dbg_sync();
            nbuf += sum_q + sum_t - nq;
            nt += sum_t;
            nq = sum_q;
            ++len;
            cur ^= 1;
        }
        // sort(haplotypes): every path takes the place of its rank
        for (uint32_t i = lane; i < nt; i += nl) {
            const uint8_t *mine = wk.hap + (uint64_t)sh->term_buf[i] * wk.hap_cap;
            uint32_t rank = 0;
            for (uint32_t j = 0; j < nt; ++j) {
                if (j == i) continue;
                const uint8_t *other = wk.hap + (uint64_t)sh->term_buf[j] * wk.hap_cap;
                if (dbg_less(other, sh->term_len[j], mine, sh->term_len[i])) ++rank;
                else if (j < i && !dbg_less(mine, sh->term_len[i], other, sh->term_len[j])) ++rank;
            }
            sh->out_buf[rank] = sh->term_buf[i];
            sh->out_len[rank] = sh->term_len[i];
        }
        dbg_sync();
        *n_out = (int)nt;
        return DBG_OK;
    }
    return DBG_NO_K;
}
