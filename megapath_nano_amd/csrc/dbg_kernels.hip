// De Bruijn graph consensus on the device (include/mpn_dbg.h): one workgroup owns a window and runs the whole of csrc/dbg_core.h on
// it -- every k from 10 upward, the k-mer table in HBM, the cycle test, pruning, the capped path walk and the sort -- without a host
// round trip per k and without waiting for another workgroup.  The host side flattens the windows, sizes one workspace per workgroup
// and runs the windows whose table or buffers turned out too small again with larger ones.
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mpn_dbg.h"
#include "dbg_core.h"
#include "mpn_common.h"

namespace {

using namespace mpn;

constexpr int DBG_THREADS = 256;
constexpr int DBG_DEFAULT_GRID = 1024;   // 4 workgroups of 256 lanes on each of the 256 CUs
constexpr int DBG_MAX_PASSES = 48;       // every pass enlarges something by 2x or more

thread_local double tl_dbg_ms = 0;

struct DbgDesc {
    uint64_t seq_off;    // of the window's bases in the flat arrays of bases and mask bytes
    uint64_t roff_off;   // of its n_reads + 1 read offsets
    uint32_t ref_len, n_reads, total, slots, hap_cap, out_index;
};

__host__ __device__ inline uint64_t align16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

// bytes of one window's workspace: the table's arrays, the reference's vertices, the run lengths, the haplotype buffers
__host__ __device__ inline uint64_t work_bytes(uint32_t slots, uint32_t ref_len, uint32_t total, uint32_t hap_cap) {
    return align16(((uint64_t)slots * 19 + ref_len) * 4) + align16(total) + align16((uint64_t)DBG_MAXP * hap_cap);
}

__global__ __launch_bounds__(DBG_THREADS) void dbg_consensus_kernel(int n, const DbgDesc *desc, const uint8_t *seq, const uint8_t *mask,
                                                                    const uint32_t *roff, uint8_t *work, uint64_t work_stride,
                                                                    int32_t *res, unsigned long long *res_off, uint8_t *arena,
                                                                    unsigned long long arena_cap, unsigned long long *arena_used) {
    __shared__ DbgShared sh;
    __shared__ unsigned long long s_off;
    const int lane = threadIdx.x;
    uint8_t *base = work + (uint64_t)blockIdx.x * work_stride;
    for (int w = blockIdx.x; w < n; w += gridDim.x) {
        const DbgDesc D = desc[w];
        DbgWindow win{seq + D.seq_off, mask + D.seq_off, roff + D.roff_off, D.ref_len, D.n_reads, D.total};
        DbgWork wk;
        const uint64_t S = D.slots;
        uint32_t *u = (uint32_t *)base;
        wk.slots = D.slots;
        wk.hap_cap = D.hap_cap;
        wk.loc = u;
        wk.succ = u + S;
        wk.pred = u + 6 * S;
        wk.w = u + 11 * S;
        wk.refmask = u + 15 * S;
        wk.indeg = u + 16 * S;
        wk.flags = u + 17 * S;
        wk.order = u + 18 * S;
        wk.refslot = u + 19 * S;
        wk.rem = base + align16((S * 19 + D.ref_len) * 4);
        wk.hap = wk.rem + align16(D.total);
        int k = 0, nh = 0;
        int status = dbg_window(win, wk, &sh, lane, DBG_THREADS, &k, &nh);
        if (status == DBG_OK && nh > 0) {
            // the window's strings: nh lengths, then the bytes back to back, at a place of their own in the pass's output
            unsigned long long bytes = 0;
            for (int i = 0; i < nh; ++i) bytes += sh.out_len[i];
            const unsigned long long need = (4ull * nh + bytes + 3) & ~3ull;
            if (lane == 0) s_off = atomicAdd(arena_used, need);
            __syncthreads();
            const unsigned long long off = s_off;
            if (off + need > arena_cap) {
                status = DBG_ARENA_FULL;
            } else {
                uint32_t *lens = (uint32_t *)(arena + off);
                uint8_t *dst = arena + off + 4ull * nh;
                for (int i = lane; i < nh; i += DBG_THREADS) lens[i] = sh.out_len[i];
                for (int i = 0; i < nh; ++i) {
                    const uint8_t *src = wk.hap + (uint64_t)sh.out_buf[i] * wk.hap_cap;
                    const uint32_t len = sh.out_len[i];
                    for (uint32_t b = lane; b < len; b += DBG_THREADS) dst[b] = src[b];
                    dst += len;
                }
                if (lane == 0) res_off[D.out_index] = off;
            }
        }
        if (lane == 0) {
            res[3 * D.out_index] = status;
            res[3 * D.out_index + 1] = k;
            res[3 * D.out_index + 2] = status == DBG_OK ? nh : 0;
        }
        __syncthreads();   // the next window reuses what the lanes share
    }
}

uint32_t pow2_at_least(uint64_t v) {
    uint32_t p = DBG_MIN_SLOTS;
    while (p < v && p < (1u << 30)) p <<= 1;
    return p;
}

struct Pending {
    int32_t window;
    uint32_t slots, hap_cap;
    int last;   // the status that sent it round again
};

int consensus_batch(int32_t n_windows, const mpn_dbg_window *windows, int64_t table_cap, int32_t grid_cap, mpn_dbg_result *out,
                    int32_t *out_redone) {
    tl_dbg_ms = 0;
    if (n_windows < 0 || table_cap < 0 || grid_cap < 0) { set_error("mpn_dbg_consensus_batch: negative count or knob"); return -2; }
    if (n_windows == 0) { if (out_redone) *out_redone = 0; return 0; }
    if (!windows || !out) { set_error("mpn_dbg_consensus_batch: NULL windows or results"); return -2; }
    // ---- refusals, all before anything is uploaded ----
    std::vector<uint8_t> seq, mask;
    std::vector<uint32_t> roff;
    std::vector<DbgDesc> all(n_windows);
    std::vector<Pending> pending(n_windows);
    uint64_t stride = 0;
    for (int32_t w = 0; w < n_windows; ++w) {
        const mpn_dbg_window &W = windows[w];
        if (!W.reference || W.n_reads < 0 || (W.n_reads > 0 && !W.reads)) {
            set_error("mpn_dbg_consensus_batch: window %d has a NULL reference or read list", w);
            return -2;
        }
        const size_t ref_len = strlen(W.reference);
        if (ref_len > MPN_DBG_MAX_REF) {
            set_error("mpn_dbg_consensus_batch: window %d has a reference of %zu bases, over the limit of %d", w, ref_len, MPN_DBG_MAX_REF);
            return -2;
        }
        DbgDesc &D = all[w];
        D.seq_off = seq.size();
        D.roff_off = roff.size();
        D.ref_len = (uint32_t)ref_len;
        D.n_reads = (uint32_t)W.n_reads;
        D.out_index = (uint32_t)w;
        seq.insert(seq.end(), (const uint8_t *)W.reference, (const uint8_t *)W.reference + ref_len);
        mask.resize(seq.size(), 0);
        uint64_t total = ref_len;
        roff.push_back((uint32_t)total);
        for (int32_t r = 0; r < W.n_reads; ++r) {
            if (!W.reads[r]) { set_error("mpn_dbg_consensus_batch: window %d, read %d is NULL", w, r); return -2; }
            const size_t len = strlen(W.reads[r]);
            total += len;
            if (total > MPN_DBG_MAX_WINDOW_BASES) {
                set_error("mpn_dbg_consensus_batch: window %d holds over %d bases", w, MPN_DBG_MAX_WINDOW_BASES);
                return -2;
            }
            seq.insert(seq.end(), (const uint8_t *)W.reads[r], (const uint8_t *)W.reads[r] + len);
            if (W.bad && W.bad[r]) mask.insert(mask.end(), W.bad[r], W.bad[r] + len);
            else mask.resize(seq.size(), 0);
            roff.push_back((uint32_t)total);
        }
        D.total = (uint32_t)total;
        // the table starts at twice the k-mers a clean window of this depth has; a noisy one comes round again
        uint32_t slots = pow2_at_least(2 * (ref_len + (total - ref_len) / 8));
        if (table_cap > 0) { uint32_t cap = DBG_MIN_SLOTS; while ((uint64_t)cap * 2 <= (uint64_t)table_cap) cap <<= 1; if (slots > cap) slots = cap; }
        pending[w] = Pending{w, slots, (uint32_t)align16(ref_len + 128), DBG_OK};
        stride = std::max(stride, work_bytes(slots, D.ref_len, D.total, pending[w].hap_cap));
    }
    if (stride > (uint64_t)MPN_DBG_WORKSPACE_BUDGET) {
        set_error("mpn_dbg_consensus_batch: a window needs a workspace of %llu bytes, over the budget of %lld", (unsigned long long)stride,
                  (long long)MPN_DBG_WORKSPACE_BUDGET);
        return -2;
    }
    // ---- upload once; then passes over what is still to do ----
    hipStream_t st = 0;
    DevBuf<uint8_t> d_seq, d_mask;
    DevBuf<uint32_t> d_roff;
    if (d_seq.upload(seq.data(), seq.size(), st) || d_mask.upload(mask.data(), mask.size(), st) || d_roff.upload(roff.data(), roff.size(), st)) return -1;
    struct Strings { int32_t status = 0, k = 0; std::vector<std::string> haps; };
    std::vector<Strings> got(n_windows);
    int32_t redone = 0;
    uint64_t arena_mult = 64;   // room for 64 haplotypes a window on average; a pass that runs out has eight times as much next time
    for (int pass = 0; !pending.empty(); ++pass) {
        if (pass == DBG_MAX_PASSES) { set_error("mpn_dbg_consensus_batch: %zu windows still unfinished after %d passes", pending.size(), pass); return -1; }
        // a window whose tables alone pass the budget is refused with its status; nothing of it was cut short
        std::vector<Pending> todo;
        stride = 0;
        uint64_t arena_cap = 4096;
        for (const Pending &p : pending) {
            const DbgDesc &D = all[p.window];
            const uint64_t b = work_bytes(p.slots, D.ref_len, D.total, p.hap_cap);
            if (b > (uint64_t)MPN_DBG_WORKSPACE_BUDGET) { got[p.window].status = p.last; got[p.window].k = 0; continue; }
            stride = std::max(stride, b);
            arena_cap += arena_mult * (D.ref_len + 64);
            todo.push_back(p);
        }
        if (todo.empty()) break;
        std::vector<DbgDesc> descs(todo.size());
        for (size_t i = 0; i < todo.size(); ++i) {
            descs[i] = all[todo[i].window];
            descs[i].slots = todo[i].slots;
            descs[i].hap_cap = todo[i].hap_cap;
            descs[i].out_index = (uint32_t)i;
        }
        uint64_t grid = std::min<uint64_t>(todo.size(), grid_cap > 0 ? grid_cap : DBG_DEFAULT_GRID);
        grid = std::max<uint64_t>(1, std::min<uint64_t>(grid, (uint64_t)MPN_DBG_WORKSPACE_BUDGET / stride));
        DevBuf<DbgDesc> d_desc;
        DevBuf<uint8_t> d_work, d_arena;
        DevBuf<int32_t> d_res;
        DevBuf<unsigned long long> d_off, d_used;
        if (d_desc.upload(descs.data(), descs.size(), st) || d_work.alloc(grid * stride) || d_arena.alloc(arena_cap) || d_res.alloc(3 * todo.size()) ||
            d_off.alloc(todo.size()) || d_used.alloc(1) || d_used.zero(st) || d_off.zero(st) || d_res.zero(st))
            return -1;
        DevTimer tm;
        if (tm.start(st)) return -1;
        hipLaunchKernelGGL(dbg_consensus_kernel, dim3((unsigned)grid), dim3(DBG_THREADS), 0, st, (int)todo.size(), (const DbgDesc *)d_desc.p,
                           (const uint8_t *)d_seq.p, (const uint8_t *)d_mask.p, (const uint32_t *)d_roff.p, d_work.p, stride, d_res.p, d_off.p,
                           d_arena.p, (unsigned long long)arena_cap, d_used.p);
        MPN_HIP_CHECK(hipGetLastError());
        if (tm.stop(st)) return -1;
        std::vector<int32_t> res(3 * todo.size());
        std::vector<unsigned long long> off(todo.size());
        unsigned long long used = 0;
        if (d_res.download(res.data(), res.size(), st) || d_off.download(off.data(), off.size(), st) || d_used.download(&used, 1, st)) return -1;
        MPN_HIP_CHECK(hipStreamSynchronize(st));
        double ms = 0;
        if (tm.elapsed_ms(&ms)) return -1;
        tl_dbg_ms += ms;
        std::vector<uint8_t> arena(std::min<uint64_t>(used, arena_cap));
        if (d_arena.download(arena.data(), arena.size(), st)) return -1;
        MPN_HIP_CHECK(hipStreamSynchronize(st));
        pending.clear();
        bool arena_full = false;
        for (size_t i = 0; i < todo.size(); ++i) {
            Pending p = todo[i];
            const int status = res[3 * i], k = res[3 * i + 1], nh = res[3 * i + 2];
            if (status == DBG_TABLE_FULL || status == DBG_HAP_FULL || status == DBG_ARENA_FULL) {
                if (status == DBG_TABLE_FULL) p.slots = p.slots < (1u << 29) ? p.slots * 4 : p.slots * 2;
                if (status == DBG_HAP_FULL) p.hap_cap *= 2;
                if (status == DBG_ARENA_FULL) arena_full = true; else p.last = status;
                if (p.slots == 0 || p.hap_cap > (1u << 30)) { got[p.window].status = status; continue; }   // (past every real window)
                pending.push_back(p);
                ++redone;
                continue;
            }
            Strings &g = got[p.window];
            g.status = status;
            g.k = k;
            if (nh < 0 || nh > DBG_MAXP || (nh > 0 && off[i] + 4ull * nh > arena.size())) { set_error("mpn_dbg_consensus_batch: a result outside the output"); return -1; }
            const uint8_t *lens = arena.data() + off[i], *bytes = lens + 4ull * nh;
            for (int h = 0; h < nh; ++h) {
                uint32_t len;
                memcpy(&len, lens + 4 * h, 4);
                if ((uint64_t)(bytes - arena.data()) + len > arena.size()) { set_error("mpn_dbg_consensus_batch: a result outside the output"); return -1; }
                g.haps.emplace_back((const char *)bytes, len);
                bytes += len;
            }
        }
        if (arena_full) arena_mult *= 8;
    }
    // ---- hand over: nothing is written before everything is there ----
    for (int32_t w = 0; w < n_windows; ++w) {
        const Strings &g = got[w];
        out[w].status = g.status;
        out[w].k = g.k;
        out[w].n_haps = (int32_t)g.haps.size();
        out[w].haps = nullptr;
        if (g.haps.empty()) continue;
        out[w].haps = (char **)malloc(g.haps.size() * sizeof(char *));
        for (size_t h = 0; h < g.haps.size(); ++h) {
            out[w].haps[h] = (char *)malloc(g.haps[h].size() + 1);
            memcpy(out[w].haps[h], g.haps[h].c_str(), g.haps[h].size() + 1);
        }
    }
    if (out_redone) *out_redone = redone;
    return 0;
}

}  // namespace

extern "C" int mpn_dbg_consensus_batch(int32_t n_windows, const mpn_dbg_window *windows, int64_t table_cap, int32_t grid_cap,
                                       mpn_dbg_result *out, int32_t *out_redone) {
    return consensus_batch(n_windows, windows, table_cap, grid_cap, out, out_redone);
}

extern "C" void mpn_dbg_free_results(mpn_dbg_result *results, int32_t n) {
    if (!results) return;
    for (int32_t w = 0; w < n; ++w) {
        for (int32_t h = 0; h < results[w].n_haps && results[w].haps; ++h) free(results[w].haps[h]);
        free(results[w].haps);
        results[w].haps = nullptr;
        results[w].n_haps = 0;
    }
}

extern "C" void mpn_dbg_last_device_ms(double *kernel_ms) {
    if (kernel_ms) *kernel_ms = tl_dbg_ms;
}

// ---- the reference's entry: strings in, a fixed array of strings out (debruijn_graph.cpp's extern "C" block) ----
static void split_commas(const char *s, std::vector<std::string> &out) {   // boost::split on ',': an empty string gives one empty part
    const char *from = s;
    for (const char *p = s;; ++p) {
        if (*p == ',' || *p == 0) {
            out.emplace_back(from, p - from);
            if (*p == 0) return;
            from = p + 1;
        }
    }
}

extern "C" mpn_dbg_str_arr *get_consensus(char *reference, char *c_reads, char *c_base_quality, int read_size) {
    (void)read_size;
    if (!reference || !c_reads || !c_base_quality) { mpn::set_error("get_consensus: NULL argument"); return nullptr; }
    std::vector<std::string> reads, lists;
    split_commas(c_reads, reads);
    split_commas(c_base_quality, lists);
    if (lists.size() < reads.size()) {
        mpn::set_error("get_consensus: %zu reads but %zu lists of low-quality positions", reads.size(), lists.size());
        return nullptr;
    }
    std::vector<std::vector<uint8_t>> bad(reads.size());
    std::vector<const char *> read_p(reads.size());
    std::vector<const uint8_t *> bad_p(reads.size());
    for (size_t r = 0; r < reads.size(); ++r) {
        // the read stops at its first NUL for the reference too (it arrives as a C string)
        bad[r].assign(reads[r].size() + 1, 0);
        const char *p = lists[r].c_str();
        for (;;) {   // `while (ss >> temp)`: integers separated by white space, up to the first thing that is none
            char *end = nullptr;
            errno = 0;
            const long v = strtol(p, &end, 10);
            if (end == p || errno == ERANGE || v > 2147483647L || v < -2147483647L - 1) break;
            if (v >= 0 && (size_t)v < reads[r].size()) bad[r][v] = 1;
            p = end;
        }
        read_p[r] = reads[r].c_str();
        bad_p[r] = bad[r].data();
    }
    mpn_dbg_window win{reference, (int32_t)reads.size(), read_p.data(), bad_p.data()};
    mpn_dbg_result res{};
    if (mpn_dbg_consensus_batch(1, &win, 0, 0, &res, nullptr) != 0) return nullptr;
    if (res.status == MPN_DBG_TABLE_FULL || res.status == MPN_DBG_HAP_FULL || res.n_haps > 500) {
        mpn::set_error("get_consensus: the window's graph passes the workspace budget");
        mpn_dbg_free_results(&res, 1);
        return nullptr;
    }
    mpn_dbg_str_arr *arr = (mpn_dbg_str_arr *)calloc(1, sizeof(mpn_dbg_str_arr));
    if (!arr) { mpn::set_error("get_consensus: out of memory"); mpn_dbg_free_results(&res, 1); return nullptr; }
    arr->consensus_size = res.n_haps;
    for (int32_t h = 0; h < res.n_haps; ++h) arr->consensus[h] = res.haps[h];   // the strings change hands
    free(res.haps);
    return arr;
}

extern "C" void free_consensus(mpn_dbg_str_arr *pointer, int size) {
    if (!pointer) return;
    for (int i = 0; i < size && i < 500; ++i) free(pointer->consensus[i]);
    free(pointer);
}
