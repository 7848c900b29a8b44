// mpn_map_batch: chains -> hits -> base-level extension -> MAPQ -> PAF  (include/mpn_map.h).
//
// Device work: seed/chain kernels (map_kernels.h) and the extension kernels (ext_kernels.h).
// This file holds what touches the device or orders the stages: the workers' slots, the extension rounds (planning, DP groups,
// stitching, finishing), the hit stage's dispatch, the pipeline over sub-batches and the mpn_map_* entries.  The host-only
// logic lives in units of its own that a host compiler builds: the per-read hit bookkeeping of minimap2's hit.c and MAPQ
// (float logf, evaluated on the host so that it is libm-exact) in hit_host.cpp, the hits accumulator and its wire format in
// hits_block.cpp, the thread pool of the host phases in host_pool.cpp, and PAF / SAM text in aln_text.cpp.
// All DP windows of a batch are planned up front and run as independent GPU jobs (one wavefront each); a hit
// whose alignment z-drops is split and its remainder goes through another round.
#include "map_types.h"
#include "ext_kernels.h"
#include "fin_kernels.h"
#include "tag_kernels.h"
#include "stitch_kernels.h"
#include "plan_kernels.h"
#include "hit_kernels.h"
#include "mapper_internal.h"
#include "hit_host.h"
#include "host_pool.h"
#include "aln_text.h"
#include "../../include/mpn_map.h"
#include "../../include/mpn_ssw.h"

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <thread>
#include <pthread.h>
#include <time.h>
#include <atomic>
#include <functional>
#include <mutex>
#include <stdlib.h>
#include <string>
#include <vector>

namespace mpn {

int upload_seqs(int32_t n, const char *seqs, const int64_t *seq_off, const int32_t *seq_len, DevBuf<uint8_t> &d_seqs,
                DevBuf<int64_t> &d_off, DevBuf<int32_t> &d_len, int64_t *total_bases, hipStream_t st);
int seed_chain_device(const mpn_index *idx, const mpn_map_opt *opt, int n, const uint8_t *d_seqs, const int64_t *d_off,
                      const int32_t *d_len, const int32_t *h_len, SeedChainOut &o, StreamLease &st, const ReadSketch *pre);
int sketch_reads(int k, int w, int n, const uint8_t *d_seqs, const int64_t *d_off, const int32_t *d_len, const int32_t *h_len, ReadSketch &sk,
                 StreamLease &st);
int download_chains(int n, SeedChainOut &o, HostChains &h, PoolBuf &pin_u, PoolBuf &pin_b, StreamLease &st, int mode);
int download_chain_records(SeedChainOut &o, HostChains &h, PoolBuf &pin_u, StreamLease &st);

const char *get_error();

// per-worker resources: a device arena, grow-only scratch pools and pinned staging buffers, and the events that join the
// extension stage's side streams (the streams themselves are leased per GPU segment: StreamLease)
struct Slot {
    hipEvent_t ev_b = nullptr, ev_c = nullptr;
    Arena arena;
    PoolBuf pool_jobs, pool_P, pool_P2, pool_OFF, pool_order, pool_state, pool_CIG, pool_res, pool_redo, pool_compact, pool_used;
    PoolBuf pool_redo_ids, pool_sregs, pool_souts, pool_fin_jobs, pool_fin_out, pool_fin_cig;
    PoolBuf pool_probes, pool_sizes, pool_buckets, pool_pregs, pool_psum, pool_job_anchor, pool_splits, pool_tags;
    PoolBuf pin_segs{nullptr, 0, true}, pin_pregs{nullptr, 0, true}, pin_hits{nullptr, 0, true};
    PoolBuf pin_order{nullptr, 0, true}, pin_res{nullptr, 0, true};
    PoolBuf pin_chain_u{nullptr, 0, true}, pin_chain_b{nullptr, 0, true};
    PoolBuf pin_fin_cig{nullptr, 0, true}, pin_fin_out{nullptr, 0, true}, pin_tags{nullptr, 0, true}, pin_tag_bytes{nullptr, 0, true};
    std::vector<std::vector<SqueezeSeg>> seg_stage;   // per pool thread: the squeeze segments of the reads it handled
    size_t device_bytes() const {
        size_t h = 0;
        for (const PoolBuf *pb : {&pool_jobs, &pool_P, &pool_P2, &pool_OFF, &pool_order, &pool_state, &pool_CIG, &pool_res, &pool_redo, &pool_compact, &pool_used,
                                  &pool_redo_ids, &pool_sregs, &pool_souts, &pool_fin_jobs, &pool_fin_out, &pool_fin_cig, &pool_probes, &pool_sizes, &pool_buckets,
                                  &pool_pregs, &pool_psum, &pool_job_anchor, &pool_splits, &pool_tags})
            h += pb->cap;
        for (const auto &c : arena.chunks) h += c.cap;
        return h;
    }
    // the slot's device memory goes back to the device (a worker that sheds, or a slot that idles in this call)
    void release_device() {
        arena.release_all();
        for (PoolBuf *pb : {&pool_jobs, &pool_P, &pool_P2, &pool_OFF, &pool_order, &pool_state, &pool_CIG, &pool_res, &pool_redo, &pool_compact, &pool_used,
                            &pool_redo_ids, &pool_sregs, &pool_souts, &pool_fin_jobs, &pool_fin_out, &pool_fin_cig, &pool_probes, &pool_sizes, &pool_buckets,
                            &pool_pregs, &pool_psum, &pool_job_anchor, &pool_splits, &pool_tags})
            pb->release();
    }
};
static Slot g_slots[16];
static thread_local Slot *tl_slot = &g_slots[0];

static int g_force_kernel = 0;  // test hook: 0 auto, 1 workgroup kernel with one wave, 3 with 256+ threads, 4 strip (else band), 5 band, 6 tiled

// the second pass of a gap fill whose CIGAR failed the z-drop test: exact maximum, band (or anti-diagonal) layout
__global__ void ext_redo_patch_kernel(ExtJob *jobs, const int32_t *ids, const int32_t *layout, const int32_t *qstride,
                                      const int64_t *p_off, const int32_t *inv, int zdrop_inv, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    ExtJob &jb = jobs[ids[k]];
    jb.flag &= ~EZ_APPROX_MAX;
    if (inv[k]) { jb.flag |= EZ_INV; jb.zdrop = zdrop_inv; }   // (mm_align1: second pass with zdrop_inv when mm_test_zdrop returned 2)
    jb.layout = layout[k];
    jb.qstride = qstride[k];
    jb.p_off = p_off[k];
}

// 0..4 codes of target intervals, for the rare host-side steps (inversion probes): interval k starts at g0[k] in concatenated
// coordinates and goes to out[off[k] .. off[k + 1])
__global__ void ref_codes_kernel(RefView rv, const int64_t *g0, const int64_t *off, int n_iv, int8_t *out) {
    for (int k = blockIdx.y; k < n_iv; k += gridDim.y) {
        const int64_t n = off[k + 1] - off[k];
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
            out[off[k] + i] = (int8_t)ref_code(rv, g0[k] + i);
    }
}
// All intervals in one launch and one wait (a wait per interval is a queue round trip each): interval k is [start, start + n)
// of the target at seq_off; its codes go to out[k]
struct RefIv { int64_t seq_off; int start, n; };
static int fetch_ref_codes(const RefView &rv, const std::vector<RefIv> &iv, std::vector<std::vector<int8_t>> &out, StreamLease &st) {
    const int n_iv = (int)iv.size();
    out.resize((size_t)n_iv);
    if (n_iv == 0) return 0;
    std::vector<int64_t> tab((size_t)2 * n_iv + 1);   // [g0 of every interval | offsets of their codes, n_iv + 1]
    int64_t *g0 = tab.data(), *off = g0 + n_iv;
    int max_n = 0;
    off[0] = 0;
    for (int k = 0; k < n_iv; ++k) {
        const int n = std::max(0, iv[(size_t)k].n);
        g0[k] = iv[(size_t)k].seq_off + iv[(size_t)k].start;
        off[k + 1] = off[k] + n;
        max_n = std::max(max_n, n);
    }
    const int64_t tot = off[n_iv];
    std::vector<int8_t> codes((size_t)tot);
    if (tot > 0) {
        DevBuf<int64_t> d_tab;
        DevBuf<int8_t> d;
        if (d_tab.alloc(tab.size()) || d.alloc((size_t)tot)) return -1;
        MPN_HIP_CHECK(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(ref_codes_kernel, dim3((unsigned)std::min(64, (max_n + 255) / 256), (unsigned)std::min(n_iv, 65535)), dim3(256), 0, st,
                           rv, (const int64_t *)d_tab.p, (const int64_t *)d_tab.p + n_iv, n_iv, d.p);
        MPN_HIP_CHECK(hipGetLastError());
        MPN_HIP_CHECK(hipMemcpyAsync(codes.data(), d.p, (size_t)tot, hipMemcpyDeviceToHost, st));
        MPN_HIP_CHECK(stream_sync(st));
    }
    for (int k = 0; k < n_iv; ++k) out[(size_t)k].assign(codes.begin() + off[k], codes.begin() + off[k + 1]);
    return 0;
}
static inline int8_t host_code(char c) { c |= 0x20; return c == 'a' ? 0 : c == 'c' ? 1 : c == 'g' ? 2 : (c == 't' || c == 'u') ? 3 : 4; }
// base x of read `seq` (length rlen) on strand rev, as a 0..4 code
static inline int8_t host_qbase(const char *seq, int rlen, int rev, int x) {
    if (!rev) return host_code(seq[x]);
    const int8_t c = host_code(seq[rlen - 1 - x]);
    return c < 4 ? (int8_t)(3 - c) : (int8_t)4;
}
// local alignment scores (ksw_ll_i16 of minimap2's inversion code) of a few pairs on the GPU: the SSW kernels of this
// library compute the same recurrences with the same tie rules for the end (first reference column with a strictly larger
// column maximum, smallest read index in it); a gap of length L costs q + L * e = SSW's (q + e) + (L - 1) * e
struct LocalHit { int score, qe, te; };
static int local_scores(const mpn_map_opt *opt, const std::vector<std::vector<int8_t>> &qs, const std::vector<std::vector<int8_t>> &ts, std::vector<LocalHit> &out) {
    const int n = (int)qs.size();
    out.assign((size_t)n, LocalHit{0, -1, -1});
    if (n == 0) return 0;
    std::vector<int8_t> qb, tb;
    std::vector<int64_t> qo(n), to(n), coff(n);
    std::vector<int32_t> ql(n), tl(n), mask(n, 15), rb(n), re(n), qb1(n), qe1(n), re2(n), clen(n), status(n);
    std::vector<uint16_t> s1(n), s2(n);
    for (int i = 0; i < n; ++i) {
        qo[i] = (int64_t)qb.size(); ql[i] = (int32_t)qs[i].size(); qb.insert(qb.end(), qs[i].begin(), qs[i].end());
        to[i] = (int64_t)tb.size(); tl[i] = (int32_t)ts[i].size(); tb.insert(tb.end(), ts[i].begin(), ts[i].end());
    }
    int8_t mat[25];
    for (int i = 0; i < 4; ++i) { for (int j = 0; j < 4; ++j) mat[i * 5 + j] = (int8_t)(i == j ? opt->a : -opt->b); mat[i * 5 + 4] = (int8_t)-opt->sc_ambi; }
    for (int i = 0; i < 5; ++i) mat[20 + i] = (int8_t)-opt->sc_ambi;
    uint32_t dummy_cig[4];
    const int rc = mpn_ssw_align_batch(n, qb.data(), qo.data(), ql.data(), tb.data(), to.data(), tl.data(), mat, 5, 2, (uint8_t)(opt->q + opt->e), (uint8_t)opt->e,
                                       0, 0, 0, mask.data(), s1.data(), s2.data(), rb.data(), re.data(), qb1.data(), qe1.data(), re2.data(), dummy_cig, 4,
                                       coff.data(), clen.data(), status.data());
    if (rc) return -1;
    for (int i = 0; i < n; ++i) if (status[i] == 0) out[(size_t)i] = LocalHit{(int)s1[i], qe1[i], re[i]};
    return 0;
}

// Device-resident state of a round's DP windows: the job records, one result record per window, and the pool of compacted
// CIGAR operations; `used` = [operations in the pool, windows listed for the exact second pass, stitched operations].  They stay
// in HBM for the stitching kernel (valid until the worker's next round); nothing per window travels to the host.
struct DevRound {
    ExtJob *jobs = nullptr;
    ExtRes *res = nullptr;
    uint32_t *compact = nullptr;
    unsigned long long *used = nullptr;
    int64_t cig_cap = 0;   // CIGAR operations the round's windows can produce at most
    int n_jobs = 0;        // windows of the round (read back with the layout counters)
};

// Run one group of DP windows whose raw job records are on the device (dv.jobs[0..nj), as plan_kernel or the stage test wrote
// them): kernel choice, direction-matrix layout and launch lists are made on the device (plan_kernels.h) and a block of counters
// comes back; then the DP kernels, the traceback, the z-drop test and the rare exact second pass.  budget > 0: returns 1
// without launching any DP if the direction matrices need more than that (the caller then cuts the range).
// host views the rare host-side steps need (inversion probes): the sub-batch's reads and the targets' offsets; null for the
// stage test, which then skips the probes
struct HostSeqs { const char *seqs; const int64_t *seq_off; const int32_t *seq_len; const int64_t *tseq_off; };

static int run_job_group(const RefView &rv, const mpn_map_opt *opt, int nj_cap, const unsigned long long *d_nj, DevRound &dv, const uint8_t *d_reads,
                         const int64_t *d_read_off, const int32_t *d_read_len, int64_t budget, const HostSeqs *hs, StreamLease &st) {
    // nj_cap: an upper bound of the number of windows (the count itself is on the device, *d_nj: the planning kernel wrote it)
    if (nj_cap == 0) return 0;
    int nj = nj_cap;
    WallTimer wt;
    Slot &SL = *tl_slot;
    const int strip_scores = ext_strip_scores_ok(opt->a, -opt->b, -opt->sc_ambi, opt->q + opt->e, opt->q2 + opt->e2) ? 1 : 0;
    ExtParams prm;
    prm.sc_mch = (int8_t)opt->a; prm.sc_mis = (int8_t)-opt->b; prm.sc_n = (int8_t)-opt->sc_ambi;
    prm.q = (int8_t)opt->q; prm.e = (int8_t)opt->e; prm.q2 = (int8_t)opt->q2; prm.e2 = (int8_t)opt->e2; prm.zdrop_thres = opt->zdrop;
    prm.zdrop_inv = opt->zdrop_inv; prm.max_gap = opt->max_gap;
    const size_t order_cap = (size_t)nj + (size_t)N_STRIP * 8 + 16;   // (a strip list is padded to whole waves: at most 7 entries)
    if (SL.pool_sizes.ensure((size_t)nj * sizeof(JobSizes) + 16) || SL.pool_buckets.ensure((size_t)2 * N_BUCKETS * 4 + sizeof(LayoutTotals) + 16) ||
        SL.pool_order.ensure(order_cap * 4) || SL.pin_res.ensure(sizeof(LayoutTotals) + 96) ||
        SL.pool_redo_ids.ensure((size_t)nj * 4 + 16) || SL.pool_probes.ensure((size_t)nj * sizeof(InvProbe) + 16))
        return -1;
    struct { ExtJob *p; } d_jobs{dv.jobs};
    JobSizes *d_sizes = SL.pool_sizes.as<JobSizes>();
    int32_t *d_bcnt = SL.pool_buckets.as<int32_t>(), *d_bcur = d_bcnt + N_BUCKETS;
    LayoutTotals *d_tot = reinterpret_cast<LayoutTotals *>(d_bcnt + 2 * N_BUCKETS);
    struct { int32_t *p; } d_order{SL.pool_order.as<int32_t>()};
    // (bucket counters and the totals block are neighbours in one pool: one fill clears both; the padding of the strip lists
    // is written by the scan kernel)
    {   // one launch zeroes the bucket counters + totals and this group's two list counters (the other counters of the round's block
        // were zeroed with it at the start of the round)
        ZeroList z{};
        zero_list_push(z, d_bcnt, (size_t)2 * N_BUCKETS * 4 + sizeof(LayoutTotals));
        zero_list_push(z, dv.used + 1, 8);
        zero_list_push(z, dv.used + 5, 8);
        zero_list_push(z, dv.used + 8, 16);  // [8] windows walked by ext_bt_wave_kernel, [9] fills failed by ext_ztest_wave_kernel (this group)
        zero_list_push(z, dv.used + 7, 8);
        MPN_HIP_CHECK(zero_regions(z, st));
    }
    const int lay_grid = std::max(1, std::min((nj + 255) / 256, 256));   // (a block per CU: every block flushes its counters once)
    EvTimer evl(st);
    static const bool tiled_on = []() { const char *e = getenv("MPN_TILED"); return !e || atoi(e) != 0; }();
    // (MPN_TILE_CLASS: the tiled class of eligible windows, for the sweep of profiles/r06_tile_pipeline; 0 = one wave)
    static const int tile_pick = []() { const char *e = getenv("MPN_TILE_CLASS"); return e ? std::min(std::max(atoi(e), 0), N_TILE_CLASS - 1) : -1; }();
    hipLaunchKernelGGL(job_classify_kernel, dim3(lay_grid), dim3(256), 0, st, d_jobs.p, d_nj, strip_scores, prm, g_force_kernel ? g_force_kernel : (tiled_on ? 0 : 7),
                       tile_pick, d_sizes, d_bcnt, d_tot);
    hipLaunchKernelGGL(job_scan_kernel, dim3(1), dim3(1024), 0, st, d_sizes, d_nj, (const int32_t *)d_bcnt, d_bcur, d_tot, d_order.p);
    hipLaunchKernelGGL(job_layout_kernel, dim3(lay_grid), dim3(256), 0, st, d_jobs.p, d_nj, (const JobSizes *)d_sizes, d_bcur, d_order.p);
    MPN_HIP_CHECK(hipGetLastError());
    LayoutTotals *h_tot = SL.pin_res.as<LayoutTotals>();
    evl.mark(56);
    MPN_HIP_CHECK(hipMemcpyAsync(h_tot, d_tot, sizeof(LayoutTotals), hipMemcpyDeviceToHost, st));
    MPN_HIP_CHECK(stream_sync(st));
    evl.resolve();
    const LayoutTotals T = *h_tot;
    nj = T.n_jobs;
    dv.n_jobs = nj;
    if (nj == 0) return 0;
    if (T.too_large) { set_error("DP window too large for LDS staging (%d x %d)", T.tl_q, T.tl_t); return -4; }
    if (!dv.compact) {
        // (the compact pool holds every window's operations, and once more those of the windows that take the second pass)
        if (SL.pool_compact.ensure((size_t)T.cig_tot * 4 * 2 + 16)) return -1;
        dv.compact = SL.pool_compact.as<uint32_t>();
        dv.cig_cap = T.cig_tot;
    }
    if (budget > 0 && T.p_tot > budget && nj > 1) return 1;
    const int *cnt = T.cnt, *base = T.base;
    g_stats[4] += nj; g_stats[5] += T.cells; g_stats[31] += T.strip_cells[0] + T.strip_cells[1] + T.strip_cells[2];
    for (int c = 0; c < 3; ++c) g_stats[41 + c] += T.strip_cells[c];
    g_stats[58] += T.xstrip_cells;
    for (int c = 0; c < N_TILE_CLASS; ++c) {   // windows on the tiled strips (none under MPN_TILED=0), and per class
        g_stats[64] += cnt[L_TILE + c];
        g_stats[STAT_TILE_CLASS + c] += cnt[L_TILE + c];
    }
    if (getenv("MPN_DEBUG_JOBS")) {
        static const char *const fam[] = {"wg64", "wg", "strip", "band", "tile"};
        for (int l = 0; l < N_LISTS; ++l)
            if (cnt[l]) fprintf(stderr, "[jobs] %s list %-2d n=%d\n", fam[l < L_WG ? 0 : l < L_STRIP ? 1 : l < L_BAND ? 2 : l < L_TILE ? 3 : 4], l, cnt[l]);
    }
    if (const char *dump = getenv("MPN_DUMP_STRIPS")) {   // debug: the geometry of the strip launch lists, in launch order
        const int n_ord = base[L_BAND] - base[L_STRIP];
        std::vector<int32_t> ord(n_ord);
        std::vector<ExtJob> hj(nj);
        MPN_HIP_CHECK(hipMemcpy(ord.data(), d_order.p + base[L_STRIP], (size_t)n_ord * 4, hipMemcpyDeviceToHost));
        MPN_HIP_CHECK(hipMemcpy(hj.data(), d_jobs.p, (size_t)nj * sizeof(ExtJob), hipMemcpyDeviceToHost));
        static std::mutex mu;
        std::lock_guard<std::mutex> lk(mu);
        if (const char *all = getenv("MPN_DUMP_JOBS"))   // ... and every window of the group: list, sizes, band, flags
            if (FILE *f = fopen(all, "ab")) {
                for (int j = 0; j < nj; ++j) {
                    const int32_t rec[6] = {hj[j].cls, hj[j].qlen, hj[j].tlen, hj[j].w, hj[j].flag, hj[j].n_col};
                    fwrite(rec, 4, 6, f);
                }
                fclose(f);
            }
        if (FILE *f = fopen(dump, "ab")) {
            for (int l = L_STRIP; l < L_BAND; ++l)
                for (int k = base[l]; k < base[l + 1]; ++k) {
                    const int jid = ord[k - base[L_STRIP]];
                    const int32_t rec[4] = {strip_glc_of_list(l), jid >= 0 ? hj[jid].qlen : 0, jid >= 0 ? hj[jid].tlen : 0, jid >= 0 ? hj[jid].strip_s : 0};
                    fwrite(rec, 4, 4, f);
                }
            fclose(f);
        }
    }
    if (SL.pool_P.ensure((size_t)T.p_tot + 16) || SL.pool_OFF.ensure((size_t)T.row_tot * 2 * 4 + 16) ||
        SL.pool_state.ensure((size_t)T.state_tot + 16) || SL.pool_CIG.ensure((size_t)T.cig_tot * 4 + 16))
        return -1;
    wt.stop_into(g_stats[27]);
    struct { uint8_t *p; } P{SL.pool_P.as<uint8_t>()};
    struct { int32_t *p; } OFF{SL.pool_OFF.as<int32_t>()};
    struct { int8_t *p; } gstate{SL.pool_state.as<int8_t>()};
    struct { uint32_t *p; } CIG{SL.pool_CIG.as<uint32_t>()};
    struct { ExtRes *p; } d_res{dv.res};
    uint32_t *d_compact = dv.compact;
    unsigned long long *d_used = dv.used;   // [0] operations in the compact pool (the whole round), [1] windows listed for the second pass (this group)
    int32_t *d_redo_ids = SL.pool_redo_ids.as<int32_t>();
    InvProbe *d_probes = SL.pool_probes.as<InvProbe>();
    // one launch of launch list `l` over ord[0..n)
    auto launch_list = [&](int l, const int32_t *ord, int n, hipStream_t s) -> int {
        if (n == 0) return 0;
        if (l < L_STRIP) {   // width class (l - L_LDS) / 5: 64, 256, 512 or 1024 threads; LDS class (l - L_LDS) % 5
            const int ntc = (l - L_LDS) / 5;
            const size_t lds = std::max<size_t>((size_t)T.lds_need[(l - L_LDS) % 5], 64);
#define MPN_WG_LAUNCH(NT)                                                                                                             \
            do {                                                                                                                      \
                if (lds > 64 * 1024) MPN_HIP_CHECK(hipFuncSetAttribute((const void *)ext_dp_wg_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                hipLaunchKernelGGL(ext_dp_wg_kernel<NT>, dim3(n), dim3(NT), lds, s, d_jobs.p, ord, n, prm, d_reads, d_read_off, d_read_len, \
                                   rv, P.p, OFF.p, gstate.p, d_res.p);                                                                \
            } while (0)
            if (ntc == 0) MPN_WG_LAUNCH(64); else if (ntc == 1) MPN_WG_LAUNCH(256); else if (ntc == 2) MPN_WG_LAUNCH(512); else MPN_WG_LAUNCH(1024);
#undef MPN_WG_LAUNCH
        } else if (l < L_BAND) {  // called once per variant family (l = its first list): all its lane-group classes in ONE launch
            const int fam = (l - L_STRIP) / 48;   // 0: gap fills (approximate maximum); 1: exact (left- and right-aligned gaps)
            StripSegs segs;
            segs.n = 0;
            int blocks = 0;
            size_t lds = 0;
            const int c_lo = fam == 0 ? 0 : 3, c_hi = fam == 0 ? 3 : N_STRIP_CLASS;
            for (int glc = 2; glc >= 0; --glc)   // wide lane groups (the long windows) first
                for (int sclass = c_lo + glc; sclass < c_hi; sclass += 3) {
                    const int l0 = L_STRIP + 16 * sclass, nl = base[l0 + 16] - base[l0], per = strip_windows_per_wave(l0);
                    if (nl == 0) continue;
                    const int stride = (std::max(T.strip_lds[sclass], 16) + 3) & ~3;
                    // exact variants: a slot per anti-diagonal and the E4 table per window (+ 16: the rows that pad the last strip)
                    const int nr_stride = fam ? T.strip_nr[sclass] + 16 : 0;
                    lds = std::max(lds, (size_t)stride * per + STRIP_TAB_BYTES + (size_t)per * 8 * nr_stride);
                    segs.s[segs.n++] = StripSeg{blocks, nl, base[l0], stride, nr_stride, glc, sclass >= 6 ? 1 : 0};
                    blocks += nl / per;
                }
            if (blocks == 0) return 0;
#define MPN_STRIP_LAUNCH(EX)                                                                                                          \
            do {                                                                                                                      \
                if (lds > 64 * 1024) MPN_HIP_CHECK(hipFuncSetAttribute((const void *)ext_dp_strip_kernel<EX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                hipLaunchKernelGGL(ext_dp_strip_kernel<EX>, dim3(blocks), dim3(64), lds, s, d_jobs.p, (const int32_t *)d_order.p, segs, prm, d_reads, \
                                   d_read_off, d_read_len, rv, P.p, d_res.p);                                                         \
            } while (0)
            if (fam == 0) MPN_STRIP_LAUNCH(false); else MPN_STRIP_LAUNCH(true);
#undef MPN_STRIP_LAUNCH
        } else if (l >= L_TILE) {   // NW waves per window (tile_class_nw), the LDS of the list's largest window (ext_tile_lds_bytes)
            const int c = l - L_TILE;
            const size_t lds = (size_t)std::max(T.tile_lds[c], 64);
#define MPN_TILE_LAUNCH(S, NW)                                                                                                        \
            do {                                                                                                                      \
                if (lds > 64 * 1024) MPN_HIP_CHECK(hipFuncSetAttribute((const void *)ext_dp_tile_kernel<S, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                hipLaunchKernelGGL((ext_dp_tile_kernel<S, NW>), dim3(n), dim3(64 * NW), lds, s, d_jobs.p, ord, n, prm, d_reads, d_read_off, \
                                   d_read_len, rv, P.p, gstate.p, d_res.p, d_used + 7);                                              \
            } while (0)
            static_assert(N_TILE_CLASS == 4, "tile classes");
            if (c == 0) MPN_TILE_LAUNCH(16, 1); else if (c == 1) MPN_TILE_LAUNCH(4, 8); else if (c == 2) MPN_TILE_LAUNCH(8, 4); else MPN_TILE_LAUNCH(4, 16);
#undef MPN_TILE_LAUNCH
        } else {
            const int bvar = (l - L_BAND) / 4;
            const size_t lds = std::max<size_t>((size_t)T.band_lds[(l - L_BAND) % 4], 64);
#define MPN_BAND_LAUNCH(NW, TT)                                                                                                       \
            do {                                                                                                                      \
                if (lds > 64 * 1024) MPN_HIP_CHECK(hipFuncSetAttribute((const void *)ext_dp_band_kernel<NW, TT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
                hipLaunchKernelGGL((ext_dp_band_kernel<NW, TT>), dim3(n), dim3(NW * 64), lds, s, d_jobs.p, ord, n, prm, d_reads, d_read_off, \
                                   d_read_len, rv, P.p, d_res.p);                                                                    \
            } while (0)
            // (two slots per thread: what bounds these kernels is the latency of an anti-diagonal, i.e. the cells a thread computes in a row)
            if (bvar == 0) MPN_BAND_LAUNCH(1, 2); else if (bvar == 1) MPN_BAND_LAUNCH(2, 2); else if (bvar == 2) MPN_BAND_LAUNCH(4, 2); else MPN_BAND_LAUNCH(8, 2);
#undef MPN_BAND_LAUNCH
        }
        MPN_HIP_CHECK(hipGetLastError());
        return 0;
    };
    EvTimer ev(st);   // (takes the segment's lease: everything this group needs from before is complete, the layout was waited for)
    // The few large windows are the long pole: they go to side streams and overlap the short windows below -- if free
    // queues can be leased without waiting (a worker never waits for a lease while it holds one).  Without them they go
    // first on the worker's own stream, ahead of the strips.
    if (!SL.ev_b) {
        MPN_HIP_CHECK(hipEventCreateWithFlags(&SL.ev_b, hipEventDisableTiming));
        MPN_HIP_CHECK(hipEventCreateWithFlags(&SL.ev_c, hipEventDisableTiming));
    }
    auto on_side = [](int l) { return (l >= L_WG && l < L_STRIP) || l >= L_BAND + 8; };  // workgroup windows, 512- and 1024-slot bands, tiled strips
    bool have_tiles = false;
    for (int l = L_TILE; l < N_LISTS; ++l) have_tiles = have_tiles || cnt[l] > 0;
    bool have_side = false;
    for (int l = 0; l < L_TILE; ++l) have_side = have_side || (on_side(l) && cnt[l] > 0);
    hipStream_t extra[2] = {nullptr, nullptr};
    const int n_extra = st.try_extra((int)have_side + (int)have_tiles, extra);
    if (have_side || have_tiles) ++g_stats[n_extra ? STAT_SIDE_LEASED : STAT_SIDE_OWN];
    const hipStream_t main_st = st;
    // (tiles: a wave per window for milliseconds; on a stream of their own they overlap the band kernels instead of preceding them)
    const hipStream_t side_st = have_side && n_extra > 0 ? extra[0] : main_st;
    const hipStream_t tile_st = have_tiles && n_extra > (int)have_side ? extra[(int)have_side] : main_st;
    for (int l = L_TILE; l < N_LISTS && have_tiles; ++l)
        if (launch_list(l, d_order.p + base[l], cnt[l], tile_st)) return -1;
    for (int l = L_TILE - 1; l >= 0; --l)
        if (on_side(l) && launch_list(l, d_order.p + base[l], cnt[l], side_st)) return -1;
    // The long windows are also the long pole of the two lane-per-window kernels (traceback, z-drop test): those of the side
    // lists run on the side stream as soon as their DP is done, beside the strip DP of the main stream.
    const int side_lo[2] = {base[L_WG], base[L_BAND + 8]}, side_hi[2] = {base[L_STRIP], base[L_TILE]};
    const int tile_lo[2] = {base[L_TILE], 0}, tile_hi[2] = {base[N_LISTS], 0};
    const int main_lo[2] = {0, base[L_STRIP]}, main_hi[2] = {base[L_WG], base[L_BAND + 8]};
    // The walks of the few long windows (tile and side lists) take a wave per window: a launch of two or three waves of lanes
    // that each chase thousands of dependent loads holds its queue for the longest of them.  The main lists (tens of thousands of
    // windows that hide each other's latency) and the second pass keep a lane per window.
    // MPN_EXT_WALK = auto (this) | lane (a lane per window everywhere) | wave (a wave per window everywhere): tests, measurements
    static const int walk_mode = []() {
        const char *e = getenv("MPN_EXT_WALK");
        return !e || !strcmp(e, "auto") ? 0 : !strcmp(e, "lane") ? 1 : !strcmp(e, "wave") ? 2 : 0;
    }();
    auto launch_bt = [&](const int32_t *ord, int n, hipStream_t s, bool wave) {
        if (n <= 0) return;
        if (wave) hipLaunchKernelGGL(ext_bt_wave_kernel, dim3(n), dim3(64), 0, s, d_jobs.p, ord, n, P.p, OFF.p, CIG.p, d_compact, d_used, d_res.p, d_used + 8);
        else hipLaunchKernelGGL(ext_bt_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_jobs.p, ord, n, P.p, OFF.p, CIG.p, d_compact, d_used, d_res.p);
    };
    auto bt_ztest = [&](const int *lo, const int *hi, hipStream_t s, bool timed, bool wave) -> int {
        for (int k = 0; k < 2; ++k) launch_bt(d_order.p + lo[k], hi[k] - lo[k], s, wave);
        MPN_HIP_CHECK(hipGetLastError());
        if (timed) ev.mark(25);
        // z-drop test of the gap-fill CIGARs (the kernel skips the other windows); flagged ones are recomputed with the exact maximum
        for (int k = 0; k < 2; ++k) {
            const int n = hi[k] - lo[k];
            if (n <= 0) continue;
            if (wave) hipLaunchKernelGGL(ext_ztest_wave_kernel, dim3(n), dim3(64), 0, s, d_jobs.p, d_order.p + lo[k], n, prm, d_reads, d_read_off, d_read_len, rv, CIG.p, d_res.p,
                                         d_redo_ids, d_used + 1, d_probes, d_used + 5, d_used + 9);
            else hipLaunchKernelGGL(ext_ztest_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_jobs.p, d_order.p + lo[k], n, prm, d_reads, d_read_off, d_read_len, rv, CIG.p, d_res.p,
                                    d_redo_ids, d_used + 1, d_probes, d_used + 5);
        }
        MPN_HIP_CHECK(hipGetLastError());
        if (timed) ev.mark(26);
        return 0;
    };
    // (the long lists' walks are timed on their own where they run on the worker's own stream, the usual case on few queues:
    // [STAT_EV_WALK_LONG], and no longer inside [15])
    if (have_side || have_tiles) ev.mark(15);
    if (have_tiles) {
        if (bt_ztest(tile_lo, tile_hi, tile_st, false, walk_mode != 1)) return -1;
        if (tile_st != main_st) MPN_HIP_CHECK(hipEventRecord(SL.ev_c, tile_st));
    }
    if (bt_ztest(side_lo, side_hi, side_st, false, walk_mode != 1)) return -1;
    if (side_st != main_st) MPN_HIP_CHECK(hipEventRecord(SL.ev_b, side_st));
    if (have_side || have_tiles) ev.mark(STAT_EV_WALK_LONG);
    for (int l = N_LISTS - 1; l >= 0; --l) {  // wide before narrow, strips (the bulk) in the middle
        if (on_side(l)) continue;
        if (l == L_BAND - 1) ev.mark(15);  // the strip launches are timed on their own ([9]): the roofline kernel of bench.py
        if (l >= L_STRIP && l < L_BAND) {  // one launch per variant family: its lists are contiguous
            if (l == L_STRIP + 48) { if (launch_list(l, nullptr, 1, main_st)) return -1; ev.mark(57); }        // the exact variants (end extensions)
            else if (l == L_STRIP) { if (launch_list(l, nullptr, 1, main_st)) return -1; ev.mark(9, 38); }    // the gap fills: the roofline kernel of bench.py
        } else if (launch_list(l, d_order.p + base[l], cnt[l], main_st)) return -1;
    }
    ev.mark(15);
    if (bt_ztest(main_lo, main_hi, main_st, true, walk_mode == 2)) return -1;
    // (waits between streams this worker holds; the sync below waits for all of them and gives them back)
    if (side_st != main_st) MPN_HIP_CHECK(hipStreamWaitEvent(main_st, SL.ev_b, 0));
    if (tile_st != main_st) MPN_HIP_CHECK(hipStreamWaitEvent(main_st, SL.ev_c, 0));
    unsigned long long *h_used = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(SL.pin_res.p) + ((sizeof(LayoutTotals) + 15) & ~(size_t)15));
    MPN_HIP_CHECK(hipMemcpyAsync(h_used, d_used, 80, hipMemcpyDeviceToHost, st));   // ([8], [9]: the wave walk kernels' counters)
    wt.stop_into(g_stats[28]);
    MPN_HIP_CHECK(stream_sync(st));
    wt.stop_into(g_stats[29]);
    // second pass: the windows whose CIGAR failed the z-drop test were listed by the test kernel (in no particular order), and
    // the windows whose largest drop may hide an inversion (mm_test_zdrop's probe: rare; decided here)
    g_stats[STAT_WALK_WAVE] += (int64_t)h_used[8];
    g_stats[STAT_WALK_WAVE_FAILED] += (int64_t)h_used[9];
    if (h_used[7]) {   // tiled windows whose hand-off wait gave up (never expected): counted, and the call fails
        g_stats[STAT_TILE_GIVEUPS] += (int64_t)h_used[7];
        set_error("%llu tiled DP windows gave up waiting for their hand-off", (unsigned long long)h_used[7]);
        return -1;
    }
    std::vector<int32_t> redo((size_t)h_used[1]);
    const int n_probe = (int)h_used[5];
    if (!redo.empty() || n_probe) {
        // (rare: the job records of the group come to the host for it)
        std::vector<ExtJob> jobs((size_t)nj);
        std::vector<InvProbe> probes((size_t)n_probe);
        if (SL.pin_order.ensure(redo.size() * 4 + 16)) return -1;
        if (!redo.empty()) MPN_HIP_CHECK(hipMemcpyAsync(SL.pin_order.p, d_redo_ids, redo.size() * 4, hipMemcpyDeviceToHost, st));
        MPN_HIP_CHECK(hipMemcpyAsync(jobs.data(), d_jobs.p, (size_t)nj * sizeof(ExtJob), hipMemcpyDeviceToHost, st));
        if (n_probe) MPN_HIP_CHECK(hipMemcpyAsync(probes.data(), d_probes, (size_t)n_probe * sizeof(InvProbe), hipMemcpyDeviceToHost, st));
        MPN_HIP_CHECK(stream_sync(st));
        if (!redo.empty()) memcpy(redo.data(), SL.pin_order.p, redo.size() * 4);
        std::vector<uint8_t> is_inv((size_t)nj, 0);
        if (n_probe) {
            std::sort(probes.begin(), probes.end(), [](const InvProbe &x, const InvProbe &y) { return x.jid < y.jid; });
            std::vector<LocalHit> hits((size_t)n_probe, LocalHit{0, -1, -1});
            if (hs) {
                // the drop's query region on the opposite strand against the drop's target region (ksw_ll_i16 in minimap2)
                std::vector<std::vector<int8_t>> qv((size_t)n_probe), tv;
                std::vector<RefIv> iv((size_t)n_probe);
                for (int k = 0; k < n_probe; ++k) {
                    const InvProbe &pb = probes[(size_t)k];
                    const ExtJob &jb = jobs[(size_t)pb.jid];
                    const int q_len = pb.q1 - pb.q0, t_len = pb.t1 - pb.t0, rlen = hs->seq_len[jb.read];
                    const char *rd = hs->seqs + hs->seq_off[jb.read];
                    qv[(size_t)k].resize((size_t)q_len);
                    for (int x = 0; x < q_len; ++x) { const int8_t c = host_qbase(rd, rlen, jb.rev, jb.qs + pb.q1 - x - 1); qv[(size_t)k][(size_t)x] = c >= 4 ? (int8_t)4 : (int8_t)(3 - c); }
                    iv[(size_t)k] = RefIv{hs->tseq_off[jb.rid], jb.ts + pb.t0, t_len};
                }
                if (fetch_ref_codes(rv, iv, tv, st)) return -1;
                if (local_scores(opt, qv, tv, hits)) return -1;
            }
            for (int k = 0; k < n_probe; ++k) {
                const InvProbe &pb = probes[(size_t)k];
                const bool inv = hits[(size_t)k].score >= opt->min_chain_score * opt->a && hits[(size_t)k].score >= opt->min_dp_max;
                if (inv) is_inv[(size_t)pb.jid] = 1;
                if (inv || pb.over) redo.push_back(pb.jid);
            }
        }
        g_stats[8] += (int64_t)redo.size();
        const int nr = (int)redo.size();
        auto list_of = [&](int j) { return jobs[(size_t)j].cls & 0xff; };
        auto redo_list_of = [&](int j) { return jobs[(size_t)j].cls >> 8 & 0xff; };
        auto band_of = [&](int j) { return (jobs[(size_t)j].cls >> 16 & 0xff) - 1; };
        std::sort(redo.begin(), redo.end(), [&](int x, int y) { return redo_list_of(x) != redo_list_of(y) ? redo_list_of(x) < redo_list_of(y) : x < y; });
        // [ids | layout | qstride | inversion flag | p_off (int64)]: a strip window's second pass needs a band / anti-diagonal
        // matrix, which comes from a pool of its own (offsets are relative to the main pool's base: one flat address space)
        std::vector<int32_t> pack((size_t)nr * 6 + 2);
        const size_t off_p = ((size_t)nr * 4 + 1) & ~(size_t)1;
        int64_t *pack_off = reinterpret_cast<int64_t *>(pack.data() + off_p);
        int64_t p2_tot = 0;
        for (int k = 0; k < nr; ++k) {
            const int j = redo[k];
            const ExtJob &jb = jobs[(size_t)j];
            const int bv = band_of(j);
            pack[k] = j; pack[nr + k] = bv >= 0 ? 2 : 0; pack[2 * nr + k] = 128 << std::max(bv, 0); pack[3 * nr + k] = is_inv[(size_t)j];
            if ((list_of(j) >= L_STRIP && list_of(j) < L_BAND) || list_of(j) >= L_TILE) {   // (strip and tiled layouts are sized for themselves)
                const int64_t n_r = (int64_t)jb.qlen + jb.tlen - 1;
                pack_off[k] = -1 - p2_tot;  // resolved below, once the pool address is known
                p2_tot += ((bv >= 0 ? n_r * (128 << bv) : n_r * jb.n_col) + 15) & ~(int64_t)15;
            } else pack_off[k] = jb.p_off;
        }
        if (nr > 0) {
            if (SL.pool_P2.ensure((size_t)p2_tot + 16)) return -1;
            const int64_t p2_base = (int64_t)(SL.pool_P2.as<uint8_t>() - P.p);
            for (int k = 0; k < nr; ++k) if (pack_off[k] < 0) pack_off[k] = p2_base + (-1 - pack_off[k]);
            if (SL.pool_redo.ensure(pack.size() * 4)) return -1;
            struct { int32_t *p; } d_redo{SL.pool_redo.as<int32_t>()};
            MPN_HIP_CHECK(hipMemcpyAsync(d_redo.p, pack.data(), pack.size() * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(ext_redo_patch_kernel, dim3((nr + 255) / 256), dim3(256), 0, st, d_jobs.p, d_redo.p, d_redo.p + nr, d_redo.p + 2 * nr,
                               reinterpret_cast<const int64_t *>(d_redo.p + off_p), d_redo.p + 3 * nr, opt->zdrop_inv, nr);
            MPN_HIP_CHECK(hipGetLastError());
            ev.skip();
            for (int lo = 0; lo < nr;) {
                int hi = lo;
                while (hi < nr && redo_list_of(redo[hi]) == redo_list_of(redo[lo])) ++hi;
                if (launch_list(redo_list_of(redo[lo]), d_redo.p + lo, hi - lo, st)) return -1;
                lo = hi;
            }
            ev.mark(15);
            launch_bt(d_redo.p, nr, st, walk_mode == 2);
            if (walk_mode == 2) g_stats[STAT_WALK_WAVE] += nr;   // (the counter was read back before the second pass; its list has no padding)
            MPN_HIP_CHECK(hipGetLastError());
            ev.mark(25);
            MPN_HIP_CHECK(stream_sync(st));
        }
    }
    ev.resolve();
    wt.stop_into(g_stats[30]);
    return 0;
}

// Run the DP windows whose raw job records the caller has put at the start of the worker's job pool (SL.pool_jobs), in groups
// whose direction scratch stays under the budget (MPN_DP_BUDGET bytes, for tests).  The job records, results and compacted
// CIGARs of ALL groups stay in the worker's device pools (out); a group only borrows the direction-matrix scratch.
// block_zeroed: the caller has zeroed the whole counter block of the round (and the planning kernel has counted into [3] since)
static int run_jobs(const RefView &rv, const mpn_map_opt *opt, int nj_cap, const uint8_t *d_reads, const int64_t *d_read_off,
                    const int32_t *d_read_len, DevRound &out, const HostSeqs *hs, StreamLease &st, bool block_zeroed = false) {
    static const int64_t budget = []() { const char *e = getenv("MPN_DP_BUDGET"); return e ? std::max<int64_t>(1 << 20, atoll(e)) : (int64_t)40 << 30; }();
    Slot &SL = *tl_slot;
    if (SL.pool_res.ensure((size_t)nj_cap * sizeof(ExtRes) + 16) || SL.pool_used.ensure(128)) return -1;
    out.jobs = SL.pool_jobs.as<ExtJob>(); out.res = SL.pool_res.as<ExtRes>(); out.compact = nullptr;
    out.used = SL.pool_used.as<unsigned long long>();   // [0] compacted ops, [1] second-pass windows, [2] stitched ops, [3] windows of the round, [4] of a sub-range
    if (!block_zeroed) {   // [0..2] and [5..7]; [3], [4] carry the window counts
        MPN_HIP_CHECK(hipMemsetAsync(out.used, 0, 24, st));
        MPN_HIP_CHECK(hipMemsetAsync(out.used + 5, 0, 24, st));
    }
    const int rc = run_job_group(rv, opt, nj_cap, out.used + 3, out, d_reads, d_read_off, d_read_len, budget, hs, st);
    if (rc != 1) return rc;
    // over the budget: cut the range where the direction matrices (their offsets are in the size table) fill it
    const int nj = out.n_jobs;
    std::vector<JobSizes> sz((size_t)nj);
    MPN_HIP_CHECK(hipMemcpyAsync(sz.data(), SL.pool_sizes.p, (size_t)nj * sizeof(JobSizes), hipMemcpyDeviceToHost, st));
    MPN_HIP_CHECK(stream_sync(st));
    std::vector<int> cuts{0};
    for (int j = 1; j < nj; ++j) if (sz[(size_t)j].p - sz[(size_t)cuts.back()].p > budget) cuts.push_back(j);
    cuts.push_back(nj);
    for (size_t g = 0; g + 1 < cuts.size(); ++g) {
        DevRound dv = out;
        dv.jobs += cuts[g]; dv.res += cuts[g];
        const unsigned long long cnt = (unsigned long long)(cuts[g + 1] - cuts[g]);
        MPN_HIP_CHECK(hipMemcpyAsync(out.used + 4, &cnt, 8, hipMemcpyHostToDevice, st));   // (cnt outlives the group's first wait)
        const int r2 = run_job_group(rv, opt, (int)cnt, out.used + 4, dv, d_reads, d_read_off, d_read_len, 0, hs, st);
        if (r2) return r2 < 0 ? r2 : -1;
    }
    out.n_jobs = nj;
    return 0;
}

}  // namespace mpn

using namespace mpn;

// The planning launch of an alignment round (plan_kernels.h), for the mapper's round loop and for the stage entry
// mpn_ext_plan_batch alike: the n_sr hits d_pr of the round are cut into DP windows.  d_used: the round's counters (64 bytes,
// reset here; the window count is d_used[3]); d_jobs / d_janchor: room for cnt + 2 windows per hit.  grid_cap: 0 = the
// mapper's grid, else at most that many blocks (the tests: one block takes every hit in turn).
static int plan_enqueue(const mpn_map_opt *opt, int32_t k, const PlanReg *d_pr, int n_sr, u128 *d_a, const int32_t *d_tlens,
                        unsigned long long *d_used, ExtJob *d_jobs, int32_t *d_janchor, StitchReg *d_sr, PlanSum *d_ps, int grid_cap,
                        hipStream_t st) {
    PlanOpt po;
    po.bw = opt->bw; po.bw15 = (int)(opt->bw * 1.5 + 1.); po.min_chain_score = opt->min_chain_score; po.max_gap = opt->max_gap;
    po.min_cnt = opt->min_cnt; po.a = opt->a; po.q = opt->q; po.e = opt->e; po.zdrop = opt->zdrop; po.zdrop_inv = opt->zdrop_inv;
    po.end_bonus = opt->end_bonus; po.min_ksw_len = opt->min_ksw_len; po.k = k; po.pad = 0; po.max_sw_mat = opt->max_sw_mat;
    MPN_HIP_CHECK(hipMemsetAsync(d_used, 0, 64, st));   // every counter of the round in one fill
    int grid = std::min(n_sr, 256 * 4);
    if (grid_cap > 0) grid = std::min(grid, grid_cap);
    hipLaunchKernelGGL(plan_kernel, dim3((unsigned)grid), dim3(64), 0, st, po, d_pr, n_sr, d_a, d_tlens, d_used + 3, d_jobs, d_janchor, d_sr, d_ps);
    MPN_HIP_CHECK(hipGetLastError());
    return 0;
}

// Stitching + CIGAR fix-up + statistics of every hit aligned in this round, on the device (stitch_kernels.h, fin_kernels.h):
// the windows' CIGARs are concatenated per hit in HBM, fixed and measured there; the host gets 56 + 32 bytes per hit, and the
// fixed CIGARs only when the caller wants text (need_cigar).
static bool g_need_cigar = true;   // set per mapping call (the calls take turns: g_call_mu)

// n_sr hits of the round; their StitchReg / PlanReg / PlanSum records and the windows' anchor indices are on the device (written
// by plan_kernel); sr_base[i] = index of read i's first hit of the round, S.pending its hits.
struct RoundDev {
    const StitchReg *sregs; const PlanReg *pregs; const PlanSum *psum; const int32_t *job_anchor; const u128 *anchors;
};

// The stitching launch of an alignment round (stitch_kernels.h), for stitch_and_finish and for the stage entry mpn_stitch_batch
// alike: the windows of the n_sr hits of rd (jobs, their results and the compact CIGAR pool) are stitched into d_cig from the
// cursor *d_out_used on; a StitchOut and a FinJob per hit, a SplitRec per cut hit from the cursor *d_n_splits on.  grid_cap: 0 =
// the mapper's grid, else at most that many blocks (the tests: one block takes every hit in turn).
static int stitch_enqueue(const RoundDev &rd, int n_sr, const ExtJob *d_jobs, const ExtRes *d_res, const uint32_t *d_compact, uint32_t *d_cig,
                          unsigned long long *d_out_used, StitchOut *d_so, FinJob *d_fj, int min_cnt, SplitRec *d_splits,
                          unsigned long long *d_n_splits, int grid_cap, hipStream_t st) {
    int grid = std::min(n_sr, 256 * 32);
    if (grid_cap > 0) grid = std::min(grid, grid_cap);
    hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)grid), dim3(64), 0, st, rd.sregs, n_sr, d_jobs, d_res, d_compact, d_cig, d_out_used, d_so, d_fj,
                       rd.pregs, rd.psum, rd.job_anchor, rd.anchors, min_cnt, d_splits, d_n_splits);
    MPN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- cs / MD / =X strings of finished alignments (tag_kernels.h): host side ------------------------------------------------
// tags_enqueue launches aln_tags_wave_kernel for the listed alignments (FinJob / FinOut / fixed CIGARs resident) and queues the
// download of the per-alignment TagOut records and the pools' cursors; after the caller's wait on the stream, tags_fetch checks
// the overflow flag and downloads exactly the bytes the kernel produced.  The pools are sized from bounds the host knows
// before the launch: with M <= min(qspan, tspan) match-op columns, cs needs at most M + qspan + tspan + 2 per op bytes (three
// per mismatch, a count of a run is no longer than the run plus its ':'), MD at most M + tspan + 2 per op, and there are at
// most M + n_ops =/X ops; the kernel takes exact slices from them and flags any write that would pass one.
struct TagJobDim { int32_t id, n_ops, qspan, tspan; };
struct TagRun {
    int tags = 0, n_jobs = 0;
    std::vector<int32_t> order;
    TagOut *d_out = nullptr;
    char *d_cs = nullptr, *d_md = nullptr;
    uint32_t *d_eqx = nullptr;
    const TagOut *h_out = nullptr;
    const unsigned long long *h_cur = nullptr;
    const char *h_cs = nullptr, *h_md = nullptr;
    const uint32_t *h_eqx = nullptr;
};
static inline int norm_tags(int t) { return (t & (MPN_TAG_CS | MPN_TAG_CS_LONG | MPN_TAG_MD | MPN_TAG_EQX)) | (t & MPN_TAG_CS_LONG ? MPN_TAG_CS : 0); }

static int tags_enqueue(Slot &SL, const std::vector<TagJobDim> &dims, int n_jobs, int64_t n_ops_total, const FinJob *d_fj, const FinOut *d_fo,
                        const uint32_t *d_cig, const uint8_t *d_seqs, const int64_t *d_off, const int32_t *d_len, const RefView &rvw, int tags,
                        hipStream_t st, TagRun &tr, EvTimer *ev = nullptr) {
    constexpr int NC = 2;
    static const int kOps[NC] = {512, 4096};   // 12 bytes of LDS per op: 6 KB and 48 KB; longer CIGARs keep the positions in global scratch
    tr.tags = tags = norm_tags(tags);
    tr.n_jobs = n_jobs;
    std::vector<int32_t> lists[NC + 1];
    int64_t cs_cap = 0, md_cap = 0, eqx_cap = 0;
    for (const TagJobDim &d : dims) {
        int c = 0;
        while (c < NC && d.n_ops > kOps[c]) ++c;
        lists[c].push_back(d.id);
        const int64_t q = std::max(0, d.qspan), t = std::max(0, d.tspan), m = std::min(q, t);
        if (tags & MPN_TAG_CS) cs_cap += m + q + t + 2 * (int64_t)d.n_ops + 16;
        if (tags & MPN_TAG_MD) md_cap += m + t + 2 * (int64_t)d.n_ops + 16;
        if (tags & MPN_TAG_EQX) eqx_cap += m + d.n_ops + 4;
    }
    int base[NC + 1];
    tr.order.clear();
    for (int c = 0; c <= NC; ++c) { base[c] = (int)tr.order.size(); tr.order.insert(tr.order.end(), lists[c].begin(), lists[c].end()); }
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t o_out = 0, o_cur = up16((size_t)n_jobs * sizeof(TagOut)), o_eqx = o_cur + 64, o_pos = o_eqx + up16((size_t)eqx_cap * 4),
                 o_list = o_pos + up16(lists[NC].empty() ? 0 : (size_t)n_ops_total * 12), o_cs = o_list + up16(tr.order.size() * 4),
                 o_md = o_cs + up16((size_t)cs_cap), total = o_md + up16((size_t)md_cap);
    if (SL.pool_tags.ensure(total + 16) || SL.pin_tags.ensure(o_eqx + 16)) return -1;
    uint8_t *d = SL.pool_tags.as<uint8_t>();
    tr.d_out = reinterpret_cast<TagOut *>(d + o_out);
    unsigned long long *d_cur = reinterpret_cast<unsigned long long *>(d + o_cur);
    tr.d_eqx = reinterpret_cast<uint32_t *>(d + o_eqx);
    int32_t *d_pos = reinterpret_cast<int32_t *>(d + o_pos), *d_list = reinterpret_cast<int32_t *>(d + o_list);
    tr.d_cs = reinterpret_cast<char *>(d + o_cs);
    tr.d_md = reinterpret_cast<char *>(d + o_md);
    MPN_HIP_CHECK(hipMemsetAsync(d, 0, o_eqx, st));   // alignments that are not listed have no strings; cursors and flag start at 0
    if (!tr.order.empty()) {
        MPN_HIP_CHECK(hipMemcpyAsync(d_list, tr.order.data(), tr.order.size() * 4, hipMemcpyHostToDevice, st));
        if (ev) ev->skip();   // (the span charged to the kernel holds its launches alone, not the memset and the list's upload)
        for (int c = 0; c < NC; ++c)
            if (!lists[c].empty())
                hipLaunchKernelGGL(aln_tags_wave_kernel<true>, dim3((unsigned)std::min<size_t>(lists[c].size(), 256 * 64)), dim3(64), (size_t)kOps[c] * 12, st, d_fj, d_fo,
                                   (const int32_t *)d_list + base[c], (int)lists[c].size(), d_cig, (int32_t *)nullptr, d_seqs, d_off, d_len, rvw, tags, tr.d_cs,
                                   (long long)cs_cap, tr.d_md, (long long)md_cap, tr.d_eqx, (long long)eqx_cap, d_cur, tr.d_out);
        if (!lists[NC].empty())
            hipLaunchKernelGGL(aln_tags_wave_kernel<false>, dim3((unsigned)std::min<size_t>(lists[NC].size(), 256 * 64)), dim3(64), 0, st, d_fj, d_fo,
                               (const int32_t *)d_list + base[NC], (int)lists[NC].size(), d_cig, d_pos, d_seqs, d_off, d_len, rvw, tags, tr.d_cs,
                               (long long)cs_cap, tr.d_md, (long long)md_cap, tr.d_eqx, (long long)eqx_cap, d_cur, tr.d_out);
        MPN_HIP_CHECK(hipGetLastError());
    }
    MPN_HIP_CHECK(hipMemcpyAsync(SL.pin_tags.p, d, o_eqx, hipMemcpyDeviceToHost, st));
    tr.h_out = SL.pin_tags.as<TagOut>();
    tr.h_cur = reinterpret_cast<const unsigned long long *>(SL.pin_tags.as<uint8_t>() + o_cur);
    return 0;
}

// after the stream has been waited for: the strings themselves (the used part of each pool), waits for them
template <typename Stream> static int tags_fetch(Slot &SL, TagRun &tr, Stream &st) {
    if (tr.h_cur[TAGC_OVERFLOW]) { set_error("difference-string kernel: an output would have passed its slice (cs %llu, MD %llu bytes, %llu =/X ops used)", tr.h_cur[TAGC_CS], tr.h_cur[TAGC_MD], tr.h_cur[TAGC_EQX]); return -1; }
    const size_t n_cs = (size_t)tr.h_cur[TAGC_CS], n_md = (size_t)tr.h_cur[TAGC_MD], n_eqx = (size_t)tr.h_cur[TAGC_EQX];
    const size_t o_cs = n_eqx * 4, o_md = o_cs + n_cs;
    if (SL.pin_tag_bytes.ensure(o_md + n_md + 16)) return -1;
    uint8_t *h = SL.pin_tag_bytes.as<uint8_t>();
    if (n_eqx) MPN_HIP_CHECK(hipMemcpyAsync(h, tr.d_eqx, n_eqx * 4, hipMemcpyDeviceToHost, st));
    if (n_cs) MPN_HIP_CHECK(hipMemcpyAsync(h + o_cs, tr.d_cs, n_cs, hipMemcpyDeviceToHost, st));
    if (n_md) MPN_HIP_CHECK(hipMemcpyAsync(h + o_md, tr.d_md, n_md, hipMemcpyDeviceToHost, st));
    if (n_eqx + n_cs + n_md) MPN_HIP_CHECK(stream_sync(st));
    tr.h_eqx = reinterpret_cast<const uint32_t *>(h);
    tr.h_cs = reinterpret_cast<const char *>(h + o_cs);
    tr.h_md = reinterpret_cast<const char *>(h + o_md);
    return 0;
}

// ---- the finishing kernel (fin_kernels.h): host side -----------------------------------------------------------------------
// fin_enqueue builds the launch lists of aln_finish_wave_kernel by LDS need (CIGAR, shift table, both code arrays: three LDS
// classes, the rest works in global scratch; a fourth class of 152 KB for the longest alignments runs them faster but blocks
// whole CUs: -2 % under the full pipeline) and launches them on st.  dims: the alignments to finish (FinJob / CIGARs resident,
// every one with at least one op); n_ops_total: the size of the CIGAR pool.  fr keeps the scratch the launches use: it must
// outlive the caller's wait on the stream.  fr.order: the alignments in launch order.  force_class (tests): 0 by need, 1..3 that
// LDS class for every alignment (refused if one does not fit), 4 the global-scratch instantiation for all.
struct FinRun {
    std::vector<int32_t> order;
    DevBuf<uint32_t> d_aux;
    DevBuf<uint8_t> d_codes;
    DevBuf<int64_t> d_code_offs;
    DevBuf<int32_t> d_list;
};

static int fin_enqueue(const std::vector<TagJobDim> &dims, int64_t n_ops_total, const mpn_map_opt *opt, const FinJob *d_fj, FinOut *d_fo,
                       uint32_t *d_cig, const uint8_t *d_seqs, const int64_t *d_off, const int32_t *d_len, const RefView &rvw, int force_class,
                       hipStream_t st, FinRun &fr, EvTimer *ev = nullptr) {
    constexpr int NC = 3;
    static const size_t kLds[NC] = {(size_t)16 << 10, (size_t)32 << 10, (size_t)64 << 10};
    if (force_class < 0 || force_class > NC + 1) { set_error("finishing kernel: force_class %d is none of 0..%d", force_class, NC + 1); return -1; }
    std::vector<int32_t> lists[NC + 1];
    std::vector<int64_t> code_offs;
    int64_t code_bytes = 0;
    for (const TagJobDim &d : dims) {
        const size_t codes = (size_t)((std::max(0, d.qspan) + 3) & ~3) + (size_t)((std::max(0, d.tspan) + 3) & ~3);
        const size_t need = (size_t)d.n_ops * 8 + codes + 16;
        int c = 0;
        if (force_class == 0) { while (c < NC && need > kLds[c]) ++c; }
        else {
            c = force_class - 1;
            if (c < NC && need > kLds[c]) { set_error("finishing kernel: alignment %d needs %zu bytes, more than the forced LDS class of %zu", d.id, need, kLds[c]); return -1; }
        }
        if (c == NC) { code_offs.push_back(code_bytes); code_bytes += (int64_t)codes; }
        lists[c].push_back(d.id);
    }
    int base[NC + 1];
    fr.order.clear();
    for (int c = 0; c <= NC; ++c) { base[c] = (int)fr.order.size(); fr.order.insert(fr.order.end(), lists[c].begin(), lists[c].end()); }
    if (fr.order.empty()) return 0;
    if (!lists[NC].empty() && (fr.d_aux.alloc((size_t)n_ops_total + 1) || fr.d_codes.alloc((size_t)code_bytes + 16) || fr.d_code_offs.upload(code_offs.data(), code_offs.size(), st)))
        return -1;
    if (fr.d_list.upload(fr.order.data(), fr.order.size(), st)) return -1;
    FinParams prm;
    for (int i = 0; i < 4; ++i) { for (int j = 0; j < 4; ++j) prm.mat[i * 5 + j] = (int8_t)(i == j ? opt->a : -opt->b); prm.mat[i * 5 + 4] = (int8_t)-opt->sc_ambi; }
    for (int i = 0; i < 5; ++i) prm.mat[20 + i] = (int8_t)-opt->sc_ambi;
    prm.q = (int8_t)opt->q; prm.e = (int8_t)opt->e;
    if (ev) ev->skip();   // (the span charged to the kernel holds its launches alone, not the uploads)
    MPN_HIP_CHECK(hipFuncSetAttribute((const void *)aln_finish_wave_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds[NC - 1]));
    for (int c = 0; c < NC; ++c)
        if (!lists[c].empty())
            hipLaunchKernelGGL(aln_finish_wave_kernel<true>, dim3((unsigned)std::min<size_t>(lists[c].size(), 256 * 64)), dim3(64), kLds[c], st, d_fj,
                               (const int32_t *)fr.d_list.p + base[c], (int)lists[c].size(), d_cig, (uint32_t *)nullptr, (uint8_t *)nullptr, d_seqs, d_off, d_len, rvw, prm, d_fo,
                               (const int64_t *)nullptr);
    if (!lists[NC].empty())
        hipLaunchKernelGGL(aln_finish_wave_kernel<false>, dim3((unsigned)std::min<size_t>(lists[NC].size(), 256 * 64)), dim3(64), 0, st, d_fj,
                           (const int32_t *)fr.d_list.p + base[NC], (int)lists[NC].size(), d_cig, fr.d_aux.p, fr.d_codes.p, d_seqs, d_off, d_len, rvw, prm, d_fo,
                           (const int64_t *)fr.d_code_offs.p);
    MPN_HIP_CHECK(hipGetLastError());
    return 0;
}

static int stitch_and_finish(const mpn_index *idx, const mpn_map_opt *opt, ReadState *rs, int n, const int32_t *seq_len, const DevRound &dv,
                             const RoundDev &rd, const std::vector<int32_t> &sr_base, const uint8_t *d_seqs, const int64_t *d_off, const int32_t *d_len,
                             int n_threads, StreamLease &st) {
    const int n_sr = sr_base[(size_t)n];
    if (n_sr == 0) return 0;
    Slot &SL = *tl_slot;
    if (SL.pin_fin_out.ensure((size_t)n_sr * (sizeof(StitchOut) + sizeof(FinOut) + sizeof(SplitRec)) + 128) ||
        SL.pool_souts.ensure((size_t)n_sr * sizeof(StitchOut) + 16) || SL.pool_splits.ensure((size_t)n_sr * sizeof(SplitRec) + 16) ||
        SL.pool_fin_jobs.ensure((size_t)n_sr * sizeof(FinJob) + 16) || SL.pool_fin_out.ensure((size_t)n_sr * sizeof(FinOut) + 16) ||
        SL.pool_fin_cig.ensure((size_t)dv.cig_cap * 4 + 16))
        return -1;
    StitchOut *d_so = SL.pool_souts.as<StitchOut>();
    FinJob *d_fj = SL.pool_fin_jobs.as<FinJob>();
    FinOut *d_fo = SL.pool_fin_out.as<FinOut>();
    uint32_t *d_cig = SL.pool_fin_cig.as<uint32_t>();
    unsigned long long *d_out_used = dv.used + 2;
    StitchOut *h_so = SL.pin_fin_out.as<StitchOut>();
    FinOut *h_fo = reinterpret_cast<FinOut *>(h_so + n_sr);
    unsigned long long *h_out_used = reinterpret_cast<unsigned long long *>(h_fo + n_sr);   // the counter block as read back
    SplitRec *h_splits = reinterpret_cast<SplitRec *>(h_out_used + 8);
    SplitRec *d_splits = SL.pool_splits.as<SplitRec>();
    unsigned long long *d_n_splits = dv.used + 6;
    EvTimer ev(st);
    ev.skip();
    if (stitch_enqueue(rd, n_sr, (const ExtJob *)dv.jobs, (const ExtRes *)dv.res, (const uint32_t *)dv.compact, d_cig, d_out_used, d_so, d_fj,
                       opt->min_cnt, d_splits, d_n_splits, 0, st))
        return -1;
    ev.mark(54);
    MPN_HIP_CHECK(hipMemcpyAsync(h_so, d_so, (size_t)n_sr * sizeof(StitchOut), hipMemcpyDeviceToHost, st));
    MPN_HIP_CHECK(hipMemcpyAsync(h_out_used, dv.used, 64, hipMemcpyDeviceToHost, st));   // the round's counter block: [2] stitched ops, [6] cut hits
    MPN_HIP_CHECK(stream_sync(st));
    const int64_t n_ops = (int64_t)h_out_used[2];
    const unsigned long long n_cut = h_out_used[6];
    if (n_cut) {   // (the cut hits' records: rare)
        MPN_HIP_CHECK(hipMemcpyAsync(h_splits, d_splits, (size_t)n_cut * sizeof(SplitRec), hipMemcpyDeviceToHost, st));
        MPN_HIP_CHECK(stream_sync(st));
    }
    // hits: coordinates, score, splits at z-drops
    parallel_for(n, n_threads, [&](int i, int) {
        ReadState &S = rs[i];
        if (S.pending.empty()) return;
        int shift = 0;
        for (size_t pi = 0; pi < S.pending.size(); ++pi) {
            const int k = S.pending[pi] + shift, fi = sr_base[(size_t)i] + (int)pi;
            Reg r2;
            const bool has = apply_stitch(seq_len[i], S.regs[(size_t)k], r2, h_splits, h_so[fi], fi);
            if (has) { S.regs.insert(S.regs.begin() + k + 1, r2); ++shift; }
        }
    }, 4);
    // hits without operations have nothing to fix (what update_extra leaves for an empty CIGAR)
    std::vector<TagJobDim> fin_dims;
    for (int j = 0; j < n_sr; ++j) {
        const StitchOut &so = h_so[j];
        if (so.n_ops == 0 || !so.has_p) continue;
        fin_dims.push_back({j, so.n_ops, so.qe1 - so.qs1, so.re1 - so.rs1});
    }
    const int out_tags = g_need_cigar ? norm_tags(opt->out_tags) : 0;   // nothing is launched, allocated or copied without them
    const bool want_tags = out_tags != 0, want_eqx = (out_tags & MPN_TAG_EQX) != 0;
    TagRun tr;
    FinRun fr;
    const RefView rvw{idx->d_seq2.p, idx->d_seq_off.p, idx->d_nrun_s.p, idx->d_nrun_e.p, idx->n_nruns};
    if (fin_enqueue(fin_dims, n_ops, opt, d_fj, d_fo, d_cig, d_seqs, d_off, d_len, rvw, 0, st, fr, &ev)) return -1;
    const std::vector<int32_t> &order = fr.order;
    if (!order.empty()) {
        ev.mark(52);
        if (want_tags) {   // cs / MD / =X of the round's alignments, while their part of the target set is resident (tag_kernels.h)
            std::vector<TagJobDim> dims;
            dims.reserve(order.size());
            for (int32_t j : order) dims.push_back({j, h_so[j].n_ops, h_so[j].qe1 - h_so[j].qs1, h_so[j].re1 - h_so[j].rs1});
            if (tags_enqueue(SL, dims, n_sr, n_ops, d_fj, d_fo, d_cig, d_seqs, d_off, d_len, rvw, opt->out_tags, st, tr, &ev)) return -1;
            ev.mark(STAT_K_TAGS);
        }
        MPN_HIP_CHECK(hipMemcpyAsync(h_fo, d_fo, (size_t)n_sr * sizeof(FinOut), hipMemcpyDeviceToHost, st));
        if (g_need_cigar && !want_eqx) {   // (with =/X CIGARs asked for, those come back instead)
            if (SL.pin_fin_cig.ensure((size_t)n_ops * 4 + 16)) return -1;
            MPN_HIP_CHECK(hipMemcpyAsync(SL.pin_fin_cig.p, d_cig, (size_t)n_ops * 4, hipMemcpyDeviceToHost, st));
        }
        MPN_HIP_CHECK(stream_sync(st));
        if (want_tags && tags_fetch(SL, tr, st)) return -1;
    }
    ev.resolve();
    g_stats[53] += n_ops;
    const uint32_t *h_cig = SL.pin_fin_cig.as<uint32_t>();
    parallel_for(n, n_threads, [&](int i, int) {
        for (Reg &r : rs[i].regs) {
            if (r.fin_idx < 0) continue;
            const StitchOut &so = h_so[r.fin_idx];
            if (so.n_ops == 0) { r.blen = r.mlen = 0; r.dp_max = 0; r.fin_idx = -1; continue; }   // (what update_extra leaves for an empty CIGAR)
            const FinOut &f = h_fo[r.fin_idx];
            if (g_need_cigar && !want_eqx) r.cigar.assign(h_cig + so.cig_off, h_cig + so.cig_off + f.n_cigar);
            if (want_tags && so.has_p) {
                const TagOut &to = tr.h_out[r.fin_idx];
                if (want_eqx) r.cigar.assign(tr.h_eqx + to.eqx_off, tr.h_eqx + to.eqx_off + to.n_eqx);
                if (out_tags & MPN_TAG_CS) r.cs.assign(tr.h_cs + to.cs_off, (size_t)to.cs_len);
                if (out_tags & MPN_TAG_MD) r.md.assign(tr.h_md + to.md_off, (size_t)to.md_len);
            }
            if (f.qshift) { if (r.rev) r.qe -= f.qshift; else r.qs += f.qshift; }
            r.rs += f.tshift;
            r.blen = f.blen; r.mlen = f.mlen; r.n_ambi += f.n_ambi; r.dp_max = f.dp_max;
            r.fin_idx = -1;
        }
    }, 9);
    return 0;
}

// What the chain stage leaves on the device for the hit stage: per read the number of its chains and where they and their
// anchors start in the compact pools, the (score, count) words, the chain records and the chained anchors.
struct HitChainsDev {
    const int32_t *n_chain; const int64_t *u_pos, *b_pos; const uint64_t *u; const ChainRec *recs; const u128 *chained;
};
// Device buffers of the hit stage that its caller reads afterwards: the squeezed anchor lists (a, sq_off) serve the alignment rounds.
struct HitStageBufs {
    DevBuf<HitRec> regs;
    DevBuf<SqueezeSeg> segs;
    DevBuf<unsigned char> reads;   // [counters (4 x 8 bytes) | HitRead[n]]
    DevBuf<u128> a;
    DevBuf<int64_t> sq_off;
};

// The hit stage of n reads: fills rs[i].regs / rs[i].n_a, sq_off (pinned, [n + 1]) and, with opt->with_cigar, the squeezed lists B.a.
// path 0: the mapper's dispatch (both instantiations of hit_select_kernel, the host above max_chains); 1: the large instantiation
// for every read of at most max_chains chains; 2: the host functions for every read (h holds the chain records then).
// o: where the records of the reads left to the host are fetched from; null when h holds them already.
// grid_cap > 0 bounds the blocks of every launch (the stage test makes a block take many reads).
static int hits_from_chains(const mpn_map_opt *opt, int k, int n, const HitChainsDev &dc, HostChains &h, SeedChainOut *o, const int32_t *seq_len,
                            const int32_t *d_len, const uint32_t *d_name_hash, const char *const *names, int path, int max_chains, int grid_cap,
                            int n_threads, StreamLease &st, ReadState *rs, HitStageBufs &B, int64_t *&sq_off, WallTimer &wt) {
    const bool gpu_hits = path != 2;
    // Hits from chains.  hit_select_kernel (hit_kernels.h) makes them on the GPU from the chain records and leaves the squeeze
    // segments there too; the host receives the selected hits (72 bytes each) and 24 bytes per read.  The chained anchors never
    // leave HBM.  Reads with more chains than the kernel stages (and every read under path 2) take the host path: the same
    // functions of hit.c on the downloaded records, their segments uploaded behind the kernel's.
    Slot &SL = *tl_slot;
    const int64_t n_chains_all = h.chain_off[(size_t)n];
    if (SL.pin_segs.ensure((size_t)n_chains_all * sizeof(SqueezeSeg) + (size_t)(n + 1) * 8 + 64)) return -1;
    sq_off = SL.pin_segs.as<int64_t>();                                     // [n + 1] start of every read's squeezed list
    SqueezeSeg *h_segs = reinterpret_cast<SqueezeSeg *>(sq_off + n + 1);
    const HitRead *h_reads = nullptr;
    const HitRec *h_hregs = nullptr;
    unsigned long long hit_counters[4] = {0, 0, 0, 0};
    if (B.segs.alloc((size_t)n_chains_all + 1)) return -1;
    if (gpu_hits && n_chains_all > 0) {
        const size_t reads_bytes = 32 + (size_t)n * sizeof(HitRead);
        if (B.regs.alloc((size_t)n_chains_all + 1) || B.reads.alloc(reads_bytes) || SL.pin_hits.ensure(reads_bytes + (size_t)n_chains_all * sizeof(HitRec) + 64)) return -1;
        MPN_HIP_CHECK(hipMemsetAsync(B.reads.p, 0, 32, st));
        HitSelParams hp;
        hp.mask_level = opt->mask_level; hp.pri_ratio = opt->pri_ratio; hp.min_join_flank_ratio = opt->min_join_flank_ratio;
        hp.min_diff = k * 2; hp.best_n = opt->best_n; hp.max_join_long = opt->max_join_long; hp.max_join_short = opt->max_join_short;
        hp.min_join_flank_sc = opt->min_join_flank_sc; hp.min_cnt = opt->min_cnt; hp.with_cigar = opt->with_cigar; hp.seed_mix = wang32(opt->seed);
        hp.max_chains = std::max(0, std::min(HIT_MAX_CHAINS, max_chains));
        EvTimer evh(st);
        // two instantiations: reads with few chains (nearly all reads of a random target set) need little LDS, so many waves per CU
#define MPN_HIT_LAUNCH(NN, LO, GRID)                                                                                                      \
        hipLaunchKernelGGL(hit_select_kernel<NN>, dim3((unsigned)std::max(1, std::min(n, grid_cap > 0 ? std::min(grid_cap, GRID) : GRID))), dim3(64), 0, st, hp, LO, n, dc.n_chain, \
                           dc.u_pos, dc.b_pos, dc.u, dc.recs, d_len, \
                           d_name_hash, B.regs.p, B.segs.p, reinterpret_cast<unsigned long long *>(B.reads.p),                \
                           reinterpret_cast<HitRead *>(B.reads.p + 32))
        if (path == 0) {
            MPN_HIT_LAUNCH(HIT_SMALL_CHAINS, 0, 256 * 16);
            MPN_HIT_LAUNCH(HIT_MAX_CHAINS, HIT_SMALL_CHAINS, 256 * 3);
        } else {   // (the stage test: the large instantiation takes the reads of the small one too)
            MPN_HIT_LAUNCH(HIT_MAX_CHAINS, 0, 256 * 3);
        }
#undef MPN_HIT_LAUNCH
        MPN_HIP_CHECK(hipGetLastError());
        evh.mark(62);
        unsigned char *pin = SL.pin_hits.as<unsigned char>();
        MPN_HIP_CHECK(hipMemcpyAsync(pin, B.reads.p, reads_bytes, hipMemcpyDeviceToHost, st));
        MPN_HIP_CHECK(stream_sync(st));
        evh.resolve();
        memcpy(hit_counters, pin, 32);
        h_reads = reinterpret_cast<const HitRead *>(pin + 32);
        HitRec *dst = reinterpret_cast<HitRec *>(pin + ((reads_bytes + 15) & ~(size_t)15));
        if (hit_counters[0]) MPN_HIP_CHECK(hipMemcpyAsync(dst, B.regs.p, (size_t)hit_counters[0] * sizeof(HitRec), hipMemcpyDeviceToHost, st));
        if (hit_counters[2] && o && download_chain_records(*o, h, SL.pin_chain_u, st)) return -1;   // reads left to the host
        MPN_HIP_CHECK(stream_sync(st));
        h_hregs = dst;
        g_stats[63] += (int64_t)hit_counters[2];
    } else if (!gpu_hits) {   // every read with chains takes the host path
        int64_t with_chains = 0;
        for (int i = 0; i < n; ++i) with_chains += h.n_chain[i] > 0;
        g_stats[63] += with_chains;
    }
    // (every pool thread stages the segments of its reads in a list of its own: a shared cursor is a hot cache line)
    std::vector<std::vector<SqueezeSeg>> &stage = SL.seg_stage;
    if ((int)stage.size() < std::max(1, n_threads)) stage.resize((size_t)std::max(1, n_threads));
    for (auto &v : stage) v.clear();
    parallel_for(n, n_threads, [&](int i, int slot) {
        ReadState &S = rs[i];
        const int nc = h.n_chain[i];
        if (nc == 0) return;
        const int qlen = seq_len[i];
        if (h_reads && h_reads[i].n_regs >= 0) {
            // the kernel's hits: the rest of the record follows from the first and last anchor (mm_reg_set_coor)
            const HitRead &hr = h_reads[i];
            const HitRec *src = h_hregs + hr.reg_pos;
            S.regs.assign((size_t)hr.n_regs, Reg());
            for (int k = 0; k < hr.n_regs; ++k) {
                Reg &r = S.regs[(size_t)k];
                const HitRec &x = src[k];
                r.id = k; r.parent = x.parent; r.score = x.score; r.score0 = x.score0; r.hash = x.hash; r.cnt = x.cnt; r.as = x.as;
                r.subsc = x.subsc; r.n_sub = x.n_sub; r.mlen = x.mlen; r.blen = x.blen;
                r.fx = x.fx; r.fy = x.fy; r.lx = x.lx; r.ly = x.ly;
                reg_set_coor(r, qlen);
            }
            if (hr.flags & 1) set_sam_pri(S.regs);
            S.n_a = hr.n_a;
            return;
        }
        CpuSect sect(g_cpu_on);
        static thread_local std::vector<ChainIn> cin;
        std::vector<int32_t> &order = tl_hs.order;
        std::vector<int64_t> &src = tl_hs.src;
        order.resize((size_t)nc); src.resize((size_t)nc); cin.resize((size_t)nc);
        h.chain_order(i, order.data(), src.data());
        for (int c = 0; c < nc; ++c) cin[c] = ChainIn{h.u_all[h.u_pos[i] + order[c]], h.rec_all + h.u_pos[i] + order[c], src[c]};
        sect.lap(3);
        uint32_t hash = names && names[i] ? x31_hash(names[i]) : 0;
        hash ^= wang32((uint32_t)qlen) + wang32(opt->seed);
        hash = wang32(hash);
        gen_regs(hash, qlen, nc, cin.data(), S.regs);
        set_parent(opt->mask_level, S.regs, opt->a * 2 + opt->b);
        select_sub(opt->pri_ratio, k * 2, opt->best_n, S.regs);
        sect.lap(4);
        std::vector<SqueezeSeg> &segs = stage[(size_t)slot % stage.size()];
        const size_t seg0 = segs.size();
        S.n_a = squeeze_a(S.regs, i, h.b_pos[i], segs);
        join_long(opt, qlen, S.regs, segs);
        if (!opt->with_cigar) segs.resize(seg0);
        sect.lap(5);
    }, 1, 128);
    int64_t n_host_segs = 0;
    for (auto &v : stage) { if (!v.empty()) memcpy(h_segs + n_host_segs, v.data(), v.size() * sizeof(SqueezeSeg)); n_host_segs += (int64_t)v.size(); }
    const int64_t n_dev_segs = (int64_t)hit_counters[1], n_segs = n_dev_segs + n_host_segs;
    wt.stop_into(g_stats[19]);
    sq_off[0] = 0;
    for (int i = 0; i < n; ++i) sq_off[i + 1] = sq_off[i] + rs[i].n_a;
    const int64_t n_sq = sq_off[n];
    if (opt->with_cigar && n_sq > 0) {
        if (B.a.alloc((size_t)n_sq) || B.sq_off.alloc((size_t)n + 1)) return -1;
        MPN_HIP_CHECK(hipMemcpyAsync(B.sq_off.p, sq_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
        // (the host's segments go behind the kernel's in the device list)
        if (n_host_segs) MPN_HIP_CHECK(hipMemcpyAsync(B.segs.p + n_dev_segs, h_segs, (size_t)n_host_segs * sizeof(SqueezeSeg), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(anchor_squeeze_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n_segs + 3) / 4, grid_cap > 0 ? std::min(grid_cap, 256 * 16) : 256 * 16))), dim3(256), 0, st,
                           (const SqueezeSeg *)B.segs.p, (int)n_segs, dc.chained, (const int64_t *)B.sq_off.p, B.a.p);
        MPN_HIP_CHECK(hipGetLastError());
        g_stats[59] += n_sq;
    }
    return 0;
}

// One contiguous range [lo, hi) of the batch through the whole path, on the calling worker's stream and arena.
// Fills rs[lo..hi) (the final hits of every read) and rep_len[lo..hi).
static int map_range(const mpn_index *idx, const mpn_map_opt *opt, const char *const *names, const char *seqs,
                     const int64_t *seq_off_all, const int32_t *seq_len_all, const uint8_t *d_seqs_p, const int64_t *d_off_all,
                     const int32_t *d_len_all, const uint32_t *d_name_hash_all, int lo, int hi, int n_threads, StreamLease &st,
                     std::vector<ReadState> &rs_all, std::vector<int32_t> &rep_len_all, const ReadSketch *sketch) {
    const int n = hi - lo;
    if (n <= 0) return 0;
    const int64_t *seq_off = seq_off_all + lo;
    const int32_t *seq_len = seq_len_all + lo;
    struct { const uint8_t *p; } d_seqs{d_seqs_p};
    struct { const int64_t *p; } d_off{d_off_all + lo};
    struct { const int32_t *p; } d_len{d_len_all + lo};
    ReadState *rs = rs_all.data() + lo;
    WallTimer wt;
    HostChains h;
    SeedChainOut o;   // (the chained anchors stay in its device pool until the squeeze below)
    bool gpu_hits = true;
    {
        // The seed + sort + chain stage is bound by HBM traffic and latency, the extension stage by VALU issue: workers in
        // different stages share the GPU well, workers in the same memory-bound stage only queue on HBM.  At most
        // MPN_SEED_SLOTS workers are inside this stage at a time (which also keeps the workers out of lock-step).
        struct StageGate {
            std::mutex mu; std::condition_variable cv; int free_slots;
            StageGate() { const char *e = getenv("MPN_SEED_SLOTS"); free_slots = e ? std::max(1, atoi(e)) : 8; }
            void enter() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return free_slots > 0; }); --free_slots; }
            void leave() { { std::lock_guard<std::mutex> g(mu); ++free_slots; } cv.notify_one(); }
        };
        static StageGate gate;
        MPN_HIP_CHECK(stream_sync(st));   // (no lease is held while waiting at the gate: the gate is entered before the lease is taken)
        struct Hold { StageGate &g; Hold(StageGate &x) : g(x) { g.enter(); } ~Hold() { g.leave(); } } hold(gate);
        if (seed_chain_device(idx, opt, n, d_seqs.p, d_off.p, d_len.p, seq_len, o, st, sketch)) return -1;
        wt.stop_into(g_stats[17]);
        // MPN_HOST_HITS=1 (tests): hits from chains on the host for every read, from the downloaded chain records
        static const bool host_hits = []() { const char *e = getenv("MPN_HOST_HITS"); return e && atoi(e) != 0; }();
        gpu_hits = !host_hits;
        if (download_chains(n, o, h, tl_slot->pin_chain_u, tl_slot->pin_chain_b, st, gpu_hits ? 0 : 1)) return -1;
        wt.stop_into(g_stats[18]);
    }
    g_stats[3] += h.chain_off[n];
    for (int i = 0; i < n; ++i) rep_len_all[lo + i] = h.rep_len[i];
    Slot &SL = *tl_slot;
    HitStageBufs hb;
    int64_t *sq_off = nullptr;   // [n + 1] start of every read's squeezed list
    {
        static const int hit_max = []() { const char *e = getenv("MPN_HIT_MAX_CHAINS"); return e ? std::max(0, std::min(HIT_MAX_CHAINS, atoi(e))) : HIT_MAX_CHAINS; }();
        const HitChainsDev dc{o.n_chain.p, o.u_pos.p, o.b_pos.p, o.u_compact.p, o.recs.p, o.chained.p};
        if (hits_from_chains(opt, idx->k, n, dc, h, &o, seq_len, d_len.p, d_name_hash_all + lo, names ? names + lo : nullptr, gpu_hits ? 0 : 2, hit_max, 0,
                             n_threads, st, rs, hb, sq_off, wt))
            return -1;
    }
    const int64_t n_sq = sq_off[n];
    if (opt->with_cigar && n_sq > 0) {
        DevBuf<u128> &d_a = hb.a;
        const RefView rv{idx->d_seq2.p, idx->d_seq_off.p, idx->d_nrun_s.p, idx->d_nrun_e.p, idx->n_nruns};
        const HostSeqs hseqs{seqs, seq_off, seq_len, idx->seq_off.data()};
        std::vector<int32_t> sr_base((size_t)n + 1, 0);
        // a round aligns every pending hit; a hit cut at a z-drop leaves a remainder with fewer anchors for the next round (minimap2 aligns it
        // in the same loop), so round k sees no hit with more anchors than the most any read has, minus k, and the last round allowed
        // finds nothing pending: one 60-kb read under scores that z-drop every few hundred bases takes well over a hundred rounds
        int64_t max_rounds = 1;
        for (int i = 0; i < n; ++i) max_rounds = std::max<int64_t>(max_rounds, (int64_t)rs[i].n_a + 1);
        bool rounds_done = false;
        for (int64_t round = 0; round < max_rounds; ++round) {
            wt.stop_into(g_stats[23]);
            // the hits to align in this round: 40 bytes each go up; their windows are planned, laid out, computed, traced back and
            // stitched on the device
            parallel_for(n, n_threads, [&](int i, int) {
                ReadState &S = rs[i];
                S.pending.clear();
                for (int k = 0; k < (int)S.regs.size(); ++k) {
                    Reg &r = S.regs[(size_t)k];
                    if (r.aligned) continue;
                    if (r.cnt == 0) { r.aligned = 1; continue; }
                    S.pending.push_back(k);
                }
            }, 2);
            for (int i = 0; i < n; ++i) sr_base[(size_t)i + 1] = sr_base[(size_t)i] + (int32_t)rs[i].pending.size();
            const int n_sr = sr_base[(size_t)n];
            if (n_sr == 0) { wt.stop_into(g_stats[20]); rounds_done = true; break; }
            std::vector<int64_t> cap_t((size_t)std::max(1, n_threads), 0);
            if (SL.pin_pregs.ensure((size_t)n_sr * sizeof(PlanReg) + 64) || SL.pool_pregs.ensure((size_t)n_sr * sizeof(PlanReg) + 16) ||
                SL.pool_psum.ensure((size_t)n_sr * sizeof(PlanSum) + 16) || SL.pool_sregs.ensure((size_t)n_sr * sizeof(StitchReg) + 16) || SL.pool_used.ensure(128))
                return -1;
            PlanReg *h_pr = SL.pin_pregs.as<PlanReg>();
            parallel_for(n, n_threads, [&](int i, int slot) {
                const ReadState &S = rs[i];
                for (size_t pi = 0; pi < S.pending.size(); ++pi) {
                    const Reg &r = S.regs[(size_t)S.pending[pi]];
                    h_pr[(size_t)sr_base[(size_t)i] + pi] = PlanReg{sq_off[i], S.n_a, r.as, r.cnt, r.mlen, i, seq_len[i], (int32_t)r.split_inv, 0};
                    cap_t[(size_t)slot % cap_t.size()] += r.cnt + 2;   // a hit of cnt anchors has at most cnt + 1 windows
                }
            }, 3);
            int64_t nj_cap64 = 0;
            for (int64_t c : cap_t) nj_cap64 += c;
            if (nj_cap64 > 0x7fffffff) { set_error("too many DP windows in one round"); return -1; }
            const int nj_cap = (int)nj_cap64;
            if (SL.pool_jobs.ensure((size_t)nj_cap * sizeof(ExtJob) + 16) || SL.pool_job_anchor.ensure((size_t)nj_cap * 4 + 16)) return -1;
            PlanReg *d_pr = SL.pool_pregs.as<PlanReg>();
            PlanSum *d_ps = SL.pool_psum.as<PlanSum>();
            StitchReg *d_sr = SL.pool_sregs.as<StitchReg>();
            ExtJob *d_jobs = SL.pool_jobs.as<ExtJob>();
            int32_t *d_janchor = SL.pool_job_anchor.as<int32_t>();
            unsigned long long *d_used = SL.pool_used.as<unsigned long long>();
            MPN_HIP_CHECK(hipMemcpyAsync(d_pr, h_pr, (size_t)n_sr * sizeof(PlanReg), hipMemcpyHostToDevice, st));
            EvTimer evp(st);
            if (plan_enqueue(opt, idx->k, d_pr, n_sr, d_a.p, idx->d_lens.p, d_used, d_jobs, d_janchor, d_sr, d_ps, 0, st)) return -1;
            evp.mark(55);
            wt.stop_into(g_stats[20]);
            ++g_stats[7];
            DevRound dv;
            if (run_jobs(rv, opt, nj_cap, d_seqs.p, d_off.p, d_len.p, dv, &hseqs, st, true)) return -1;
            evp.resolve();
            if (!dv.compact) {   // (a round without any window: the stitching kernel still sets the hits' coordinates)
                if (SL.pool_compact.ensure(64)) return -1;
                dv.compact = SL.pool_compact.as<uint32_t>();
            }
            wt.stop_into(g_stats[21]);
            const RoundDev rd{d_sr, d_pr, d_ps, d_janchor, d_a.p};
            if (stitch_and_finish(idx, opt, rs, n, seq_len, dv, rd, sr_base, d_seqs.p, d_off.p, d_len.p, n_threads, st)) return -1;
            wt.stop_into(g_stats[22]);
        }
        if (!rounds_done) { set_error("hits still unaligned after the last alignment round"); return -1; }   // (never: no hit without CIGAR leaves quietly)
        // ---- inversions (mm_align1_inv): where a hit was cut at an inversion, the read's gap between the two pieces is aligned
        // to the target's gap on the opposite strand.  Rare; the candidates are gathered on the host, the local alignment that
        // locates the inverted segment runs on the SSW kernels, its extension is one more (tiny) round of the DP pipeline.
        struct InvCand { int read, at, ql, tl, rev, qstart, tstart, rid; };
        std::vector<InvCand> cand;
        for (int i = 0; i < n; ++i) {
            const std::vector<Reg> &R = rs[i].regs;
            for (int k = 1; k < (int)R.size(); ++k) {
                if (!R[(size_t)k].split_inv) continue;
                const Reg &r1 = R[(size_t)k - 1], &r2 = R[(size_t)k];
                if (!(r1.split & 1) || !(r2.split & 2)) continue;
                if (r1.id != r1.parent && r1.parent != PARENT_TMP_PRI) continue;
                if (r2.id != r2.parent && r2.parent != PARENT_TMP_PRI) continue;
                if (r1.rid != r2.rid || r1.rev != r2.rev) continue;
                const int ql = r1.rev ? r1.qs - r2.qe : r2.qs - r1.qe, tl = r2.rs - r1.re;
                if (ql < opt->min_chain_score || ql > opt->max_gap || tl < opt->min_chain_score || tl > opt->max_gap) continue;
                // the read's gap on the strand opposite to the hit: forward coordinates from r2.qe if the hit is on the reverse
                // strand, reverse-strand coordinates from qlen - r2.qs otherwise
                cand.push_back(InvCand{i, k, ql, tl, r1.rev ? 0 : 1, r1.rev ? r2.qe : seq_len[i] - r2.qs, r1.re, r1.rid});
            }
        }
        if (!cand.empty()) {
            const int nc = (int)cand.size();
            std::vector<std::vector<int8_t>> qv((size_t)nc), tv;
            std::vector<RefIv> iv((size_t)nc);
            for (int c = 0; c < nc; ++c) {   // both sequences reversed: the best local alignment's END there is its START here
                const InvCand &ic = cand[(size_t)c];
                const char *rd_ = seqs + seq_off[ic.read];
                qv[(size_t)c].resize((size_t)ic.ql);
                for (int x = 0; x < ic.ql; ++x) qv[(size_t)c][(size_t)x] = host_qbase(rd_, seq_len[ic.read], ic.rev, ic.qstart + ic.ql - 1 - x);
                iv[(size_t)c] = RefIv{idx->seq_off[(size_t)ic.rid], ic.tstart, ic.tl};
            }
            if (fetch_ref_codes(rv, iv, tv, st)) return -1;
            for (auto &t : tv) std::reverse(t.begin(), t.end());
            std::vector<LocalHit> lh;
            if (local_scores(opt, qv, tv, lh)) return -1;
            std::vector<ExtJob> jobs;
            std::vector<StitchReg> sregs;
            for (int i = 0; i < n; ++i) rs[i].pending.clear();
            // placeholders go in from the back of every read's list, so that the positions of the earlier candidates stay valid
            for (int c = nc - 1; c >= 0; --c) {
                const InvCand &ic = cand[(size_t)c];
                if (lh[(size_t)c].score < opt->min_dp_max) continue;
                const int q_off = ic.ql - (lh[(size_t)c].qe + 1), t_off = ic.tl - (lh[(size_t)c].te + 1);
                Reg ri;
                ri.id = -1; ri.parent = PARENT_UNSET; ri.inv = 1; ri.rev = (uint32_t)ic.rev; ri.rid = ic.rid; ri.cnt = 0; ri.aligned = 0;
                ri.fin_qs = ic.qstart + q_off; ri.fin_rs = ic.tstart + t_off; ri.fin_ql = ic.ql - q_off; ri.fin_tl = ic.tl - t_off;
                rs[ic.read].regs.insert(rs[ic.read].regs.begin() + ic.at + 1, ri);
            }
            for (int i = 0; i < n; ++i) {
                std::vector<Reg> &R = rs[i].regs;
                for (int k = 0; k < (int)R.size(); ++k) {
                    Reg &r = R[(size_t)k];
                    if (!r.inv || r.aligned) continue;
                    rs[i].pending.push_back(k);
                    ExtJob j;
                    memset(&j, 0, sizeof(j));
                    j.read = i; j.rid = r.rid; j.rev = (int32_t)r.rev; j.qs = r.fin_qs; j.qlen = r.fin_ql; j.ts = r.fin_rs; j.tlen = r.fin_tl; j.reversed = 0;
                    j.w = (int)(opt->bw * 1.5); j.zdrop = opt->zdrop; j.end_bonus = -1; j.flag = EZ_EXTZ_ONLY; j.strip_s = 1; j.cls = -1;
                    sregs.push_back(StitchReg{(int32_t)jobs.size(), 1, j.qs, j.ts, j.qs, j.ts, j.qs, j.qs + j.qlen, i, r.rid, (int32_t)r.rev, 0});
                    jobs.push_back(j);
                }
            }
            if (!jobs.empty()) {
                const int nj = (int)jobs.size();
                for (int i = 0; i < n; ++i) sr_base[(size_t)i + 1] = sr_base[(size_t)i] + (int32_t)rs[i].pending.size();
                if (SL.pool_jobs.ensure((size_t)nj * sizeof(ExtJob) + 16) || SL.pool_sregs.ensure((size_t)nj * sizeof(StitchReg) + 16) ||
                    SL.pool_pregs.ensure(64) || SL.pool_psum.ensure(64) || SL.pool_job_anchor.ensure(64) || SL.pool_used.ensure(128))
                    return -1;
                const unsigned long long cnt = (unsigned long long)nj;
                MPN_HIP_CHECK(hipMemcpyAsync(SL.pool_jobs.p, jobs.data(), (size_t)nj * sizeof(ExtJob), hipMemcpyHostToDevice, st));
                MPN_HIP_CHECK(hipMemcpyAsync(SL.pool_sregs.p, sregs.data(), (size_t)nj * sizeof(StitchReg), hipMemcpyHostToDevice, st));
                MPN_HIP_CHECK(hipMemcpyAsync(SL.pool_used.as<unsigned long long>() + 3, &cnt, 8, hipMemcpyHostToDevice, st));
                MPN_HIP_CHECK(stream_sync(st));
                DevRound dv;
                if (run_jobs(rv, opt, nj, d_seqs.p, d_off.p, d_len.p, dv, &hseqs, st)) return -1;
                if (!dv.compact) { if (SL.pool_compact.ensure(64)) return -1; dv.compact = SL.pool_compact.as<uint32_t>(); }
                const RoundDev rd{SL.pool_sregs.as<StitchReg>(), SL.pool_pregs.as<PlanReg>(), SL.pool_psum.as<PlanSum>(), SL.pool_job_anchor.as<int32_t>(), d_a.p};
                if (stitch_and_finish(idx, opt, rs, n, seq_len, dv, rd, sr_base, d_seqs.p, d_off.p, d_len.p, n_threads, st)) return -1;
            }
            // an extension that produced nothing yields no inversion hit (mm_align1_inv returns 0)
            for (int i = 0; i < n; ++i) {
                std::vector<Reg> &R = rs[i].regs;
                R.erase(std::remove_if(R.begin(), R.end(), [](const Reg &r) { return r.inv && !r.has_p; }), R.end());
            }
        }
    }
    wt.stop_into(g_stats[23]);
    // rank, MAPQ, text
    std::atomic<int64_t> n_aln(0);
    parallel_for(n, n_threads, [&](int i, int) {
        ReadState &S = rs[i];
        const int qlen = seq_len[i];
        if (!S.regs.empty()) {
            if (opt->with_cigar) {
                filter_regs(opt, qlen, S.regs);
                hit_sort(S.regs);
                set_parent(opt->mask_level, S.regs, opt->a * 2 + opt->b);
                select_sub(opt->pri_ratio, idx->k * 2, opt->best_n, S.regs);
                set_sam_pri(S.regs);
            }
            set_mapq(S.regs, opt->min_chain_score, opt->a, h.rep_len[i]);
        }
        n_aln += (int64_t)S.regs.size();
    }, 5);
    g_stats[6] += n_aln;
    wt.stop_into(g_stats[23]);
    return 0;
}

// The mapping itself: every read's final hits against every one of n_parts RESIDENT indexes -> rs[part], rep_len[part] (no text).
// One index is the plain case.  Several are the parts of a target set that exceeds one index (minimap2 -I): the work items of
// the pipeline are (sub-batch, part) pairs, so the reads go up once, and the pipeline neither drains nor refills between parts.
static int map_batch_core(const mpn_index *const *parts, int n_parts, const mpn_map_opt *opt, int32_t n, const char *const *names, const char *seqs,
                          const int64_t *seq_off, const int32_t *seq_len, const void *r_seqs, const int64_t *r_off, const int32_t *r_len,
                          std::vector<std::vector<ReadState>> &rs, std::vector<std::vector<int32_t>> &rep_len, int *n_threads_out) {
    hipStream_t st0 = 0;
    struct Borrowed {  // device views of the reads: owned uploads or the caller's resident buffers
        DevBuf<uint8_t> seqs; DevBuf<int64_t> off; DevBuf<int32_t> len;
        const uint8_t *p = nullptr; const int64_t *po = nullptr; const int32_t *pl = nullptr;
    } dv;
    int64_t bases = 0;
    WallTimer wt;
    if (r_seqs && r_off && r_len) {
        dv.p = (const uint8_t *)r_seqs; dv.po = r_off; dv.pl = r_len;
        for (int i = 0; i < n; ++i) bases += seq_len[i];
    } else {
        if (upload_seqs(n, seqs, seq_off, seq_len, dv.seqs, dv.off, dv.len, &bases, st0)) return -1;
        dv.p = dv.seqs.p; dv.po = dv.off.p; dv.pl = dv.len.p;
    }
    // per read: the x31 hash of its name (what minimap2 mixes into the order of equal-scoring chains), for hit_select_kernel
    DevBuf<uint32_t> d_name_hash;
    {
        std::vector<uint32_t> nh((size_t)n, 0u);
        if (names) for (int i = 0; i < n; ++i) nh[(size_t)i] = names[i] ? x31_hash(names[i]) : 0u;
        if (d_name_hash.upload(nh.data(), (size_t)n, st0)) return -1;
        MPN_HIP_CHECK(hipStreamSynchronize(st0));
    }
    MPN_HIP_CHECK(hipStreamSynchronize(st0));
    wt.stop_into(g_stats[16]);
    int n_threads = default_host_threads(opt);
    *n_threads_out = n_threads;
    pool_ensure(n_threads);
    // sub-batches of ~32 Mbp run through a small pool of workers (12 by default), each with its own device arena and a
    // submission stream leased per GPU segment (StreamLease), so that the host phases of one sub-batch overlap the GPU phases of the others and the
    // latency-bound kernels (chain DP, long extensions) of one overlap the throughput-bound ones of another
    int n_workers = 12;
    if (const char *e = getenv("MPN_PIPE_WORKERS")) n_workers = std::max(1, std::min(16, atoi(e)));
    // Sub-batches: equal-sized, their count a multiple of the worker count so that no worker idles in the last round.  Every worker
    // holds its own scratch (direction matrices above all): ~400 bytes per base of a sub-batch on a random target set, several times
    // that on a strain-rich one -- what the workers of the previous calls took per sub-batch base is remembered.  When the free HBM
    // (plus what the slots hold) does not cover all workers at the default size -- several index parts resident -- the sub-batches
    // shrink (not below 11 Mbp) before workers are given up: 12 workers on 11 Mbp run 3 % faster than 6 on 22 Mbp (profiles/r04).
    static double obs_bytes_per_bp = 0.0;   // (the mapping calls take turns: g_call_mu)
    static int64_t obs_sub_bp = 0;
    const bool env_target = getenv("MPN_SUB_BATCH_BP") != nullptr;
    const int W_all = n_workers;
    std::vector<int> cut;
    auto make_cuts = [&](int64_t target) {
        cut.assign(1, 0);
        std::vector<int64_t> sizes;
        int64_t n_cut = std::max<int64_t>(1, (bases + target - 1) / target);
        if (n_cut > W_all) n_cut = (n_cut + W_all - 1) / W_all * W_all;
        for (int64_t i = 0; i < n_cut; ++i) sizes.push_back(std::max<int64_t>(1, (bases + n_cut - 1) / n_cut));
        size_t si = 0;
        int64_t acc = 0;
        for (int i = 0; i < n; ++i) {
            acc += seq_len[i];
            if (si + 1 < sizes.size() && acc >= sizes[si] && i + 1 < n) { cut.push_back(i + 1); acc = 0; ++si; }
        }
        cut.push_back(n);
    };
    int64_t target = 32000000;
    if (env_target) target = std::max<int64_t>(1000, atoll(getenv("MPN_SUB_BATCH_BP")));
    make_cuts(target);
    int n_sub = (int)cut.size() - 1;
    int64_t largest = n_sub > 0 ? (bases + n_sub - 1) / n_sub : bases;
    {
        size_t free_b = 0, total_b = 0, held = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            for (const Slot &S : g_slots) held += S.device_bytes();
            const double avail = 0.9 * (double)(free_b + held);
            // (no call has been observed yet: the need of a strain-rich multi-part target set, 850 bytes per base, is assumed -- a first call
            // sized for a random target set ran out of memory on it, shed workers and took five times a steady-state call)
            const double bytes_per_bp = obs_bytes_per_bp > 0 ? std::max(400.0, 1.15 * obs_bytes_per_bp) : 900.0;
            auto per_worker = [&](int64_t sub_bp) { return bytes_per_bp * (double)std::max<int64_t>(sub_bp, 1) + 2e9; };
            int fit = (int)std::max(1.0, avail / per_worker(largest));
            if (fit < std::min(W_all, n_sub) && !env_target && largest > 11000000) {
                // what fits W_all workers, at least 11 Mbp
                const double room = avail / W_all - 2e9;
                const int64_t t2 = std::max<int64_t>(11000000, (int64_t)(room / bytes_per_bp));
                if (t2 < largest) {
                    make_cuts(t2);
                    n_sub = (int)cut.size() - 1;
                    largest = n_sub > 0 ? (bases + n_sub - 1) / n_sub : bases;
                    fit = (int)std::max(1.0, avail / per_worker(largest));
                }
            }
            // pools that were grown for much larger sub-batches would keep the memory the smaller ones free: give them back once
            if (obs_sub_bp > 0 && largest < obs_sub_bp * 3 / 4) {
                MPN_HIP_CHECK(hipDeviceSynchronize());
                for (Slot &S : g_slots) S.release_device();
            }
            n_workers = std::min(n_workers, fit);
        }
    }
    const int n_items = n_sub;   // a work item is a sub-batch: its worker maps it against every part in turn, on ONE sketch of its reads
    n_workers = std::max(1, std::min(n_workers, n_items));
    // slots that idle in this call give their scratch back: the running workers may need it (a call with fewer workers than the
    // last one -- less free memory since another index part became resident, or MPN_PIPE_WORKERS lowered)
    for (int wdx = n_workers; wdx < 16; ++wdx)
        if (g_slots[wdx].device_bytes()) { MPN_HIP_CHECK(hipDeviceSynchronize()); g_slots[wdx].release_device(); }
    int dev = 0;
    MPN_HIP_CHECK(hipGetDevice(&dev));
    QueueStreams *qs = queue_streams(dev);   // (created once per device, before any worker runs)
    if (!qs) { set_error("creating the submission streams failed"); return -1; }
    rs.assign((size_t)n_parts, std::vector<ReadState>());
    rep_len.assign((size_t)n_parts, std::vector<int32_t>());
    for (int p = 0; p < n_parts; ++p) { rs[(size_t)p].assign((size_t)n, ReadState()); rep_len[(size_t)p].assign((size_t)n, 0); }
    std::atomic<int> next(0), failed(0);
    std::mutex mu;
    std::deque<int> retry;          // sub-batches given back by a worker that ran out of device memory (guarded by mu)
    int live_workers = n_workers, live_workers_busy = 0, n_shed = 0;   // (guarded by mu)
    int64_t tot_stats[MPN_NSTATS] = {0};
    std::string err;
    const bool dbg_workers = getenv("MPN_DEBUG_WORKERS") != nullptr;
    g_phase_log.on = getenv("MPN_DEBUG_PHASES") != nullptr;
    g_cpu_on = getenv("MPN_DEBUG_CPU") != nullptr;
    if (g_cpu_on) { for (auto &c : g_cpu_ns) c = 0; for (auto &c : g_worker_cpu_ns) c = 0; }
    g_worker_cpu_on = g_cpu_on;
    if (g_phase_log.on) { g_phase_log.recs.clear(); g_phase_log.origin = std::chrono::steady_clock::now(); }
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    auto worker = [&](int wid) {
        pthread_setname_np(pthread_self(), "mpn-work");
        if (hipSetDevice(dev) != hipSuccess) { failed = 1; return; }
        Slot &S = g_slots[wid];
        StreamLease lease(qs);
        tl_slot = &S;
        tl_arena = &S.arena;
        tl_worker_id = wid;
        memset(g_stats, 0, sizeof(g_stats));
        for (;;) {
            int sb = -1;
            { std::lock_guard<std::mutex> g(mu); if (!retry.empty()) { sb = retry.front(); retry.pop_front(); } }
            if (sb < 0) sb = next.fetch_add(1);
            if (sb >= n_items || failed) {
                // (a sub-batch may still come back from a worker that is shedding: wait for those before leaving)
                std::unique_lock<std::mutex> lk(mu);
                if (failed || (retry.empty() && live_workers_busy == 0)) break;
                lk.unlock();
                timespec ts{0, 200000};
                nanosleep(&ts, nullptr);
                continue;
            }
            { std::lock_guard<std::mutex> g(mu); ++live_workers_busy; }
            struct Busy { std::mutex &m; int &c; ~Busy() { std::lock_guard<std::mutex> g(m); --c; } } busy_{mu, live_workers_busy};
            S.arena.reset();
            tl_oom = false;
            int64_t stats_before[MPN_NSTATS];
            memcpy(stats_before, g_stats, sizeof(stats_before));
            const double t_in = since();
            struct Out { bool on; int wid, sb; double t_in; decltype(since) &f; ~Out() { if (on) fprintf(stderr, "[worker %d] sub-batch %d: %.1f -> %.1f ms\n", wid, sb, t_in, f()); } } out_{dbg_workers, wid, sb, t_in, since};
            int rc_item = 0;
            {
                ReadSketch sk;
                const int sbi = sb, nr = cut[sbi + 1] - cut[sbi];
                if (n_parts > 1 && nr > 0) {
                    WallTimer wts;
                    rc_item = sketch_reads(parts[0]->k, parts[0]->w, nr, dv.p, dv.po + cut[sbi], dv.pl + cut[sbi], seq_len + cut[sbi], sk, lease);
                    wts.stop_into(g_stats[17]);
                }
                const Arena::Mark after_sketch = S.arena.mark();
                for (int prt = 0; prt < n_parts && !rc_item; ++prt) {
                    S.arena.rewind(after_sketch);   // (what the previous part took is dead; the sketch stays)
                    rc_item = map_range(parts[prt], opt, names, seqs, seq_off, seq_len, dv.p, dv.po, dv.pl, d_name_hash.p, cut[sbi], cut[sbi + 1], n_threads, lease,
                                        rs[(size_t)prt], rep_len[(size_t)prt], sk.valid ? &sk : nullptr);
                }
                if (!rc_item && stream_sync(lease) != hipSuccess) { set_error("stream wait failed"); rc_item = -1; }
            }
            if (rc_item) {
                std::lock_guard<std::mutex> g(mu);
                // Out of device memory: the workers' scratch grows with what the target set throws at them (a strain-rich index
                // yields tens of times the anchors of a random one), and the up-front estimate can be too low.  This worker gives
                // its memory back and leaves; its sub-batch goes to the others.  The last worker standing reports the failure.
                if (tl_oom && live_workers > 1) {   // (the flag of this thread's failed device allocation, not the error text)
                    --live_workers;
                    ++n_shed;
                    memcpy(g_stats, stats_before, sizeof(stats_before));
                    (void)hipGetLastError();
                    (void)stream_sync(lease);
                    S.release_device();
                    retry.push_back(sb);
                    if (dbg_workers) fprintf(stderr, "[worker %d] out of device memory at sub-batch %d: leaving, %d workers go on\n", wid, sb, live_workers);
                    break;
                }
                err = get_error();
                failed = 1;
                (void)stream_sync(lease);
                break;
            }
        }
        tl_arena = nullptr;
        std::lock_guard<std::mutex> g(mu);
        for (int k = 0; k < MPN_NSTATS; ++k) tot_stats[k] += g_stats[k];
    };
    {
        std::vector<std::thread> th;
        for (int wdx = 0; wdx < n_workers; ++wdx) th.emplace_back(worker, wdx);
        for (auto &t : th) t.join();
    }
    if (dbg_workers) {
        fprintf(stderr, "[call] workers joined at %.1f ms\n", since());
        for (int wdx = 0; wdx < n_workers; ++wdx) {
            const Slot &S = g_slots[wdx];
            size_t arena = 0;
            for (const auto &c : S.arena.chunks) arena += c.cap;
            const size_t pools = S.pool_jobs.cap + S.pool_P.cap + S.pool_P2.cap + S.pool_OFF.cap + S.pool_order.cap + S.pool_state.cap + S.pool_CIG.cap +
                                 S.pool_res.cap + S.pool_redo.cap + S.pool_compact.cap + S.pool_used.cap;
            const size_t pinned = S.pin_order.cap + S.pin_res.cap + S.pin_chain_u.cap + S.pin_chain_b.cap + S.pin_segs.cap + S.pin_pregs.cap + S.pin_fin_cig.cap + S.pin_fin_out.cap + S.pin_tags.cap + S.pin_tag_bytes.cap;
            fprintf(stderr, "[slot %d] arena %.2f GB, pools %.2f GB (P %.2f, CIG %.2f, compact %.2f), pinned host %.2f GB\n", wdx, arena / 1e9,
                    pools / 1e9, S.pool_P.cap / 1e9, S.pool_CIG.cap / 1e9, S.pool_compact.cap / 1e9, pinned / 1e9);
        }
    }
    if (g_phase_log.on) {
        for (const auto &r : g_phase_log.recs) fprintf(stderr, "[phase] %d %d %lld %lld\n", r.worker, r.slot, (long long)r.t0, (long long)r.t1);
        fprintf(stderr, "[phase-end]\n");
    }
    if (g_cpu_on) {
        static const char *const nm[] = {"other", "hits", "plan", "plan-copy", "stitch", "final", "dp-group-A", "strip-sort", "job-copy", "finish-copy", "accumulate", "merge"};
        fprintf(stderr, "[cpu] thread CPU ms in parallel regions:");
        for (int k = 0; k < 12; ++k) fprintf(stderr, " %s %.0f", nm[k], g_cpu_ns[k].load() / 1e6);
        fprintf(stderr, "\n[cpu] sections: stitch-append %.0f", g_cpu_ns[16].load() / 1e6);
        for (int k = 3; k < 16; ++k) if (g_cpu_ns[16 + k].load() > 500000) fprintf(stderr, " s%d %.0f", k, g_cpu_ns[16 + k].load() / 1e6);
        fprintf(stderr, "\n[cpu] worker-thread CPU ms by phase slot:");
        for (int k = 0; k < 64; ++k) if (g_worker_cpu_ns[k].load() > 500000) fprintf(stderr, " [%d] %.0f", k, g_worker_cpu_ns[k].load() / 1e6);
        fprintf(stderr, "\n");
    }
    if (failed) { set_error("%s", err.empty() ? "worker failed" : err.c_str()); return -1; }
    {
        const int64_t h2d = g_stats[16];
        memcpy(g_stats, tot_stats, sizeof(tot_stats));
        g_stats[16] = h2d;
        g_stats[0] = bases;
        g_stats[60] = n_shed; g_stats[61] = n_workers;
        {   // what a worker took per sub-batch base in this call (the next call sizes its sub-batches and workers by it)
            size_t held_max = 0;
            for (const Slot &S : g_slots) held_max = std::max(held_max, S.device_bytes());
            if (largest > 0 && held_max > 0) {
                const double r = (double)held_max / (double)largest;
                obs_bytes_per_bp = obs_sub_bp == largest ? std::max(obs_bytes_per_bp, r) : r;
                obs_sub_bp = largest;
            }
        }
    }
    return 0;
}

// Text and columns of a batch whose hits are final.  opt->out_sam: 0 = PAF into text, 1 = SAM into text, 2 = PAF into text and
// SAM kept for mpn_map_fetch_sam.  Results that do not fit the caller's buffers are kept (mpn_map_fetch_cols / _text)
// so that the caller fetches them with larger buffers instead of mapping the batch again.  Returns bytes of text or -3.
static struct Kept { std::vector<int32_t> cols; int64_t n_rows = -1; std::string text, sam; bool has_text = false, has_sam = false; } g_kept;

static int64_t emit_batch(const Targets tg, const mpn_map_opt *opt, int32_t n, const char *const *names, const char *seqs, const char *quals,
                          const int64_t *seq_off, const int32_t *seq_len, std::vector<std::vector<Reg>*> &regs, const std::vector<int32_t> &rep_len,
                          int n_threads, char *text, int64_t text_cap, mpn_aln_cols *cols) {
    const bool want_paf = text && opt->out_sam != 1, want_sam = opt->out_sam == 2 || (text && opt->out_sam == 1);
    std::vector<std::string> paf_lines(want_paf ? n : 0), sam_lines(want_sam ? n : 0);
    int64_t n_aln = 0;
    for (int i = 0; i < n; ++i) n_aln += (int64_t)regs[i]->size();
    if (want_paf || want_sam)
        parallel_for(n, n_threads, [&](int i, int) {
            const char *nm = names && names[i] ? names[i] : "*";
            if (want_paf && !regs[i]->empty()) write_paf(tg, opt, nm, seq_len[i], *regs[i], rep_len[i], paf_lines[i]);
            if (want_sam) write_sam(tg, opt, nm, seq_len[i], seqs + seq_off[i], quals ? quals + seq_off[i] : nullptr, *regs[i], rep_len[i], sam_lines[i]);
        }, 0, 16);   // (text is heavy per read)
    bool short_cols = false, short_text = false;
    g_kept.cols.clear(); g_kept.text.clear(); g_kept.sam.clear(); g_kept.n_rows = -1; g_kept.has_text = g_kept.has_sam = false;
    if (cols) {
        cols->n_rows = n_aln;
        short_cols = n_aln > cols->cap;
        int32_t *dst[13] = {cols->read_idx, cols->qs, cols->qe, cols->rev, cols->rid, cols->rs, cols->re, cols->mlen, cols->blen, cols->mapq,
                            cols->nm, cols->as, cols->primary};
        if (short_cols) {
            g_kept.cols.resize((size_t)n_aln * 13);
            g_kept.n_rows = n_aln;
            for (int c = 0; c < 13; ++c) dst[c] = g_kept.cols.data() + (size_t)c * (size_t)n_aln;
        }
        int64_t k = 0;
        for (int i = 0; i < n; ++i)
            for (const Reg &r : *regs[i]) {
                dst[0][k] = i; dst[1][k] = r.qs; dst[2][k] = r.qe; dst[3][k] = (int32_t)r.rev; dst[4][k] = r.rid;
                dst[5][k] = r.rs; dst[6][k] = r.re; dst[7][k] = r.mlen; dst[8][k] = r.blen; dst[9][k] = (int32_t)r.mapq;
                dst[10][k] = r.has_p ? r.blen - r.mlen + r.n_ambi : -1;
                dst[11][k] = r.has_p ? r.dp_score : -1;
                dst[12][k] = r.id == r.parent;
                ++k;
            }
    }
    int64_t w = 0;
    if (text) {
        std::vector<std::string> &lines = opt->out_sam == 1 ? sam_lines : paf_lines;
        int64_t tot = 0;
        for (auto &l : lines) tot += (int64_t)l.size();
        short_text = tot + 1 > text_cap;
        if (short_text) {
            g_kept.text.reserve((size_t)tot);
            for (auto &l : lines) g_kept.text += l;
            g_kept.has_text = true;
        } else {
            for (auto &l : lines) { memcpy(text + w, l.data(), l.size()); w += (int64_t)l.size(); }
            text[w] = 0;
        }
    }
    if (opt->out_sam == 2) {
        size_t tot = 0;
        for (auto &l : sam_lines) tot += l.size();
        g_kept.sam.reserve(tot);
        for (auto &l : sam_lines) g_kept.sam += l;
        g_kept.has_sam = true;
    }
    parallel_chunks(n, n_threads, [&](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi; ++i) { if (want_paf) std::string().swap(paf_lines[i]); if (want_sam) std::string().swap(sam_lines[i]); }
    });
    g_stats[6] = n_aln;
    return (short_cols || short_text) ? -3 : w;
}

static std::mutex g_call_mu;  // the worker slots (streams, arenas, pools) are process-wide: concurrent callers take turns

extern "C" int64_t mpn_map_batch_q(const mpn_index *idx, const mpn_map_opt *opt, int32_t n, const char *const *names,
                                   const char *seqs, const char *quals, const int64_t *seq_off, const int32_t *seq_len, const void *r_seqs,
                                   const int64_t *r_off, const int32_t *r_len, char *paf, int64_t paf_cap, mpn_aln_cols *cols) {
    std::lock_guard<std::mutex> call_guard(g_call_mu);
    memset(g_stats, 0, sizeof(g_stats));
    if (cols) cols->n_rows = 0;
    if (n <= 0) { if (paf && paf_cap > 0) paf[0] = 0; g_kept = Kept(); if (opt->out_sam == 2) g_kept.has_sam = true; return 0; }
    WallTimer whole;
    std::vector<std::vector<ReadState>> rs_p;
    std::vector<std::vector<int32_t>> rep_p;
    int n_threads = 1;
    g_need_cigar = paf != nullptr || opt->out_sam != 0;   // columns only: the CIGARs never leave the GPU
    if (map_batch_core(&idx, 1, opt, n, names, seqs, seq_off, seq_len, r_seqs, r_off, r_len, rs_p, rep_p, &n_threads)) return -1;
    std::vector<ReadState> &rs = rs_p[0];
    std::vector<int32_t> &rep_len = rep_p[0];
    std::vector<std::vector<Reg>*> regs((size_t)n);
    for (int i = 0; i < n; ++i) regs[(size_t)i] = &rs[(size_t)i].regs;
    const int64_t w = emit_batch(Targets{&idx->names, &idx->lens}, opt, n, names, seqs, quals, seq_off, seq_len, regs, rep_len, n_threads, paf, paf_cap, cols);
    // the per-read state (regs with their CIGARs) is a few hundred thousand small allocations: free them in parallel
    parallel_chunks(n, n_threads, [&](int64_t lo, int64_t hi, int) { for (int64_t i = lo; i < hi; ++i) rs[(size_t)i] = ReadState(); });
    whole.stop_into(g_stats[24]);
    return w;
}

extern "C" int64_t mpn_map_batch_ex(const mpn_index *idx, const mpn_map_opt *opt, int32_t n, const char *const *names,
                                    const char *seqs, const int64_t *seq_off, const int32_t *seq_len, const void *r_seqs,
                                    const int64_t *r_off, const int32_t *r_len, char *paf, int64_t paf_cap, mpn_aln_cols *cols) {
    return mpn_map_batch_q(idx, opt, n, names, seqs, nullptr, seq_off, seq_len, r_seqs, r_off, r_len, paf, paf_cap, cols);
}

// ---- split index (minimap2 -I parts + --split-prefix merge) ---------------------------------------------------------
// several RESIDENT parts in one call (288 GB of HBM hold what a CPU host streams through -I): the pipeline's work items are
// (sub-batch, part) pairs; the hits land in the accumulator part by part, in the order given, as repeated
// mpn_map_batch_part calls would leave them
extern "C" int mpn_map_batch_parts(const mpn_index *const *parts, int32_t n_parts, const mpn_map_opt *opt, int32_t n, const char *const *names,
                                   const char *seqs, const int64_t *seq_off, const int32_t *seq_len, const void *r_seqs, const int64_t *r_off,
                                   const int32_t *r_len, mpn_hits *acc) {
    if (!acc || n != acc->n_reads) { set_error("mpn_map_batch_parts: the accumulator was created for another batch"); return -1; }
    if (!parts || n_parts <= 0) { set_error("mpn_map_batch_parts: no index part"); return -1; }
    for (int p = 0; p < n_parts; ++p)
        if (!parts[p] || parts[p]->k != parts[0]->k) { set_error("mpn_map_batch_parts: null part or parts built with different k"); return -1; }
    const int part_tags = acc->want_text && opt->with_cigar ? norm_tags(opt->out_tags) : 0;
    if (acc->n_parts > 0 && part_tags != acc->tags) { set_error("mpn_map_batch_parts: out_tags differs from that of the parts already accumulated"); return -1; }
    std::lock_guard<std::mutex> call_guard(g_call_mu);
    memset(g_stats, 0, sizeof(g_stats));
    if (n > 0) {
        std::vector<std::vector<ReadState>> rs;
        std::vector<std::vector<int32_t>> rep_len;
        int n_threads = 1;
        g_need_cigar = acc->want_text != 0;   // (text is asked for at mpn_hits_finish: the accumulator says whether it will be)
        if (map_batch_core(parts, n_parts, opt, n, names, seqs, seq_off, seq_len, r_seqs, r_off, r_len, rs, rep_len, &n_threads)) return -1;
        std::vector<int32_t> rid0((size_t)n_parts);
        int32_t r0 = (int32_t)acc->lens.size();
        for (int p = 0; p < n_parts; ++p) { rid0[(size_t)p] = r0; r0 += parts[p]->n_seq; }
        parallel_chunks(n, n_threads, [&](int64_t lo, int64_t hi, int) {
            for (int64_t i = lo; i < hi; ++i) {
                size_t more = 0;
                for (int p = 0; p < n_parts; ++p) more += rs[(size_t)p][(size_t)i].regs.size();
                acc->regs[(size_t)i].reserve(acc->regs[(size_t)i].size() + more);
                for (int p = 0; p < n_parts; ++p) {
                    for (Reg &r : rs[(size_t)p][(size_t)i].regs) { r.rid += rid0[(size_t)p]; acc->regs[(size_t)i].push_back(std::move(r)); }
                    acc->rep_len[(size_t)i] = std::max(acc->rep_len[(size_t)i], rep_len[(size_t)p][(size_t)i]);
                    rs[(size_t)p][(size_t)i] = ReadState();
                }
            }
        }, 10);
    }
    acc->tags = part_tags;   // (only now: a call that failed leaves no claim)
    for (int p = 0; p < n_parts; ++p) {
        acc->names.insert(acc->names.end(), parts[p]->names.begin(), parts[p]->names.end());
        acc->lens.insert(acc->lens.end(), parts[p]->lens.begin(), parts[p]->lens.end());
        acc->k = parts[p]->k;
        ++acc->n_parts;
    }
    return 0;
}

extern "C" int mpn_map_batch_part(const mpn_index *part, const mpn_map_opt *opt, int32_t n, const char *const *names, const char *seqs,
                                  const int64_t *seq_off, const int32_t *seq_len, const void *r_seqs, const int64_t *r_off,
                                  const int32_t *r_len, mpn_hits *acc) {
    return mpn_map_batch_parts(&part, 1, opt, n, names, seqs, seq_off, seq_len, r_seqs, r_off, r_len, acc);
}

extern "C" int64_t mpn_hits_finish(mpn_hits *acc, const mpn_map_opt *opt, int32_t n, const char *const *names, const char *seqs,
                                   const char *quals, const int64_t *seq_off, const int32_t *seq_len, char *paf, int64_t paf_cap,
                                   mpn_aln_cols *cols) {
    if (!acc || n != acc->n_reads) { set_error("mpn_hits_finish: the accumulator was created for another batch"); return -1; }
    std::lock_guard<std::mutex> call_guard(g_call_mu);
    if (cols) cols->n_rows = 0;
    if (n <= 0) { if (paf && paf_cap > 0) paf[0] = 0; g_kept = Kept(); if (opt->out_sam == 2) g_kept.has_sam = true; return 0; }
    const int n_threads = default_host_threads(opt);
    pool_ensure(n_threads);
    if (!acc->n_parts) { set_error("mpn_hits_finish: no part was mapped"); return -1; }
    if (!acc->want_text && (paf || opt->out_sam != 0)) { set_error("mpn_hits_finish: text asked of an accumulator that was told there would be none (mpn_hits_set_text)"); return -1; }
    if ((paf || opt->out_sam != 0) && opt->with_cigar) {   // the strings were made while the parts were resident: they cannot be made now
        const int req = norm_tags(opt->out_tags);
        if ((req & ~acc->tags) || ((req & MPN_TAG_CS) && ((req ^ acc->tags) & MPN_TAG_CS_LONG))) {
            set_error("mpn_hits_finish: out_tags 0x%x asks for output that the accumulated hits do not carry (parts were mapped with 0x%x)", req, acc->tags);
            return -1;
        }
    }
    if (g_cpu_on) { g_cpu_ns[11] = 0; g_cpu_ns[0] = 0; }
    struct Report { ~Report() { if (g_cpu_on) fprintf(stderr, "[cpu] finish: merge %.0f ms, text/other %.0f ms (thread CPU in parallel regions)\n", g_cpu_ns[11].load() / 1e6, g_cpu_ns[0].load() / 1e6); } } report_;
    parallel_for(n, n_threads, [&](int i, int) { merge_regs(opt, acc->k, acc->regs[(size_t)i], acc->rep_len[(size_t)i]); }, 11, 128);
    std::vector<std::vector<Reg>*> regs((size_t)n);
    for (int i = 0; i < n; ++i) regs[(size_t)i] = &acc->regs[(size_t)i];
    return emit_batch(Targets{&acc->names, &acc->lens}, opt, n, names, seqs, quals, seq_off, seq_len, regs, acc->rep_len, n_threads, paf, paf_cap, cols);
}

extern "C" int64_t mpn_map_fetch_cols(mpn_aln_cols *cols) {
    if (!cols || g_kept.n_rows < 0) { set_error("mpn_map_fetch_cols: no columns kept from the last call"); return -1; }
    cols->n_rows = g_kept.n_rows;
    if (cols->cap < g_kept.n_rows) return -3;
    int32_t *dst[13] = {cols->read_idx, cols->qs, cols->qe, cols->rev, cols->rid, cols->rs, cols->re, cols->mlen, cols->blen, cols->mapq,
                        cols->nm, cols->as, cols->primary};
    for (int c = 0; c < 13; ++c)
        if (g_kept.n_rows) memcpy(dst[c], g_kept.cols.data() + (size_t)c * (size_t)g_kept.n_rows, (size_t)g_kept.n_rows * 4);
    const int64_t r = g_kept.n_rows;
    std::vector<int32_t>().swap(g_kept.cols);
    g_kept.n_rows = -1;
    return r;
}

static int64_t fetch_kept(std::string &txt, bool &has, const char *what, char *buf, int64_t cap) {
    if (!has) { set_error("%s: no text kept from the last call", what); return -1; }
    const int64_t need = (int64_t)txt.size();
    if (!buf) return need + 1;  // size query
    if (cap < need + 1) return -3;
    memcpy(buf, txt.data(), (size_t)need);
    buf[need] = 0;
    std::string().swap(txt);
    has = false;
    return need;
}
extern "C" int64_t mpn_map_fetch_text(char *buf, int64_t cap) { return fetch_kept(g_kept.text, g_kept.has_text, "mpn_map_fetch_text", buf, cap); }
extern "C" int64_t mpn_map_fetch_sam(char *buf, int64_t cap) { return fetch_kept(g_kept.sam, g_kept.has_sam, "mpn_map_fetch_sam", buf, cap); }

extern "C" int64_t mpn_sam_header(const mpn_index *idx, const char *cmdline, char *buf, int64_t cap) {
    return sam_header_of(idx->names, idx->lens, cmdline, buf, cap);
}
extern "C" int64_t mpn_hits_sam_header(const mpn_hits *h, const char *cmdline, char *buf, int64_t cap) {
    return sam_header_of(h->names, h->lens, cmdline, buf, cap);
}

extern "C" int64_t mpn_map_batch(const mpn_index *idx, const mpn_map_opt *opt, int32_t n, const char *const *names, const char *seqs,
                                 const int64_t *seq_off, const int32_t *seq_len, char *paf, int64_t paf_cap) {
    return mpn_map_batch_ex(idx, opt, n, names, seqs, seq_off, seq_len, nullptr, nullptr, nullptr, paf, paf_cap, nullptr);
}

#include "stage_entries.h"
