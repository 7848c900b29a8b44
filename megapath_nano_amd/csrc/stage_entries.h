// The stage entry points of align.hip's unit (include/mpn_map.h): each checks host arrays, uploads them, launches one stage as the
// product launches it and flattens the result into plain integer rows for the parity tests.  Included once by align.hip, behind
// the product code: the entries use its file-local state (tl_slot, g_force_kernel, g_call_mu) and its launch functions.
// What they check on the host and the buffers of the pair entries come from stage_input.h, which a CPU test runs on its own.
#include "stage_input.h"

using namespace mpn_stage;

// the device half of the pair entries' input layer: a checked pair set (sp) and its buffers, the targets packed to 2 bits with a
// zero word behind them; with CIGARs also the pairs' finishing jobs and the launch dimensions of those that have ops (as in the
// product: no ops, no launch)
struct StagePairsDev {
    StagePairs sp;
    RefView rv{};
    std::vector<uint32_t> words;
    std::vector<int64_t> ns, ne;
    std::vector<FinJob> jobs;
    std::vector<TagJobDim> dims;
    DevBuf<uint8_t> d_reads;
    DevBuf<uint32_t> d_ref, d_cig;
    DevBuf<int64_t> d_qoff, d_toff, d_ns, d_ne;
    DevBuf<int32_t> d_qlen;
    DevBuf<FinJob> d_fj;
    int upload(hipStream_t st) {
        pack_2bit(sp.tcodes, sp.ttot, words, ns, ne);
        words.push_back(0);
        const size_t n = (size_t)sp.n;
        if (d_reads.upload(sp.reads.data(), sp.reads.size(), st) || d_ref.upload(words.data(), words.size(), st) || d_ns.upload(ns.data(), ns.size(), st) ||
            d_ne.upload(ne.data(), ne.size(), st) || d_qoff.upload(sp.q_off, n, st) || d_qlen.upload(sp.q_len, n, st) || d_toff.upload(sp.t_off, n, st))
            return -1;
        rv = RefView{d_ref.p, d_toff.p, d_ns.p, d_ne.p, (int32_t)ns.size()};
        return 0;
    }
    // the same for pairs with alignments, checked as stage_pairs_build checks them
    int upload_alns(const char *who, int32_t n, const uint8_t *qcodes, const int64_t *q_off, const int32_t *q_len, const int32_t *qs, const int32_t *qe,
                    const int32_t *rev, const uint8_t *tcodes, const int64_t *t_off, const int32_t *t_len, const int32_t *ts, const uint32_t *cigar,
                    const int64_t *cig_off, const int32_t *n_cigar, bool allow_empty_ops, hipStream_t st) {
        if (!stage_pairs_build(who, n, qcodes, q_off, q_len, tcodes, t_off, t_len, qs, qe, ts, cigar, cig_off, n_cigar, allow_empty_ops, set_error, sp)) return -1;
        jobs.assign((size_t)n, FinJob{});
        for (int i = 0; i < n; ++i) {
            FinJob &f = jobs[(size_t)i];
            f.cig_off = cig_off[i]; f.n_cigar = n_cigar[i]; f.read = i; f.rid = i; f.rev = rev[i] ? 1 : 0;
            f.qs1 = rev[i] ? q_len[i] - qe[i] : qs[i]; f.rs1 = ts[i]; f.qspan = sp.qspan[(size_t)i]; f.tspan = sp.tspan[(size_t)i];
            if (f.n_cigar > 0) dims.push_back({i, f.n_cigar, f.qspan, f.tspan});
        }
        return upload(st) || d_cig.upload(sp.cigar.data(), sp.cigar.size(), st) || d_fj.upload(jobs.data(), jobs.size(), st) ? -1 : 0;
    }
};

// stage entry point for the parity tests: the DP kernels on arbitrary (query, target) code pairs
extern "C" int mpn_ext_dp_batch(const mpn_map_opt *opt, int32_t n, const uint8_t *qcodes, const int64_t *q_off, const int32_t *q_len,
                                const uint8_t *tcodes, const int64_t *t_off, const int32_t *t_len, const int32_t *w,
                                const int32_t *zdrop, const int32_t *end_bonus, const int32_t *flag, int32_t force_kernel,
                                int32_t *out9, uint32_t *cigar_pool, int64_t cigar_cap, int64_t *cig_off) {
    std::lock_guard<std::mutex> call_guard(g_call_mu);
    hipStream_t st = 0;
    if (n <= 0) return 0;
    if (!opt || !qcodes || !q_off || !q_len || !tcodes || !t_off || !t_len || !w || !zdrop || !end_bonus || !flag || !out9 || !cig_off) {
        set_error("mpn_ext_dp_batch: options or an array missing"); return -1;
    }
    StagePairsDev in;
    if (!stage_pairs_build("mpn_ext_dp_batch", n, qcodes, q_off, q_len, tcodes, t_off, t_len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           false, set_error, in.sp) || in.upload(st))
        return -1;
    std::vector<ExtJob> jobs(n);
    for (int i = 0; i < n; ++i) {
        ExtJob &j = jobs[i];
        memset(&j, 0, sizeof(j));
        j.read = i; j.rid = i; j.rev = 0; j.qs = 0; j.qlen = q_len[i]; j.ts = 0; j.tlen = t_len[i]; j.reversed = 0;
        j.w = w[i]; j.zdrop = zdrop[i]; j.end_bonus = end_bonus[i]; j.flag = flag[i]; j.strip_s = 1; j.cls = -1;
    }
    struct ForceKernel {   // (back to the dispatch on every way out)
        explicit ForceKernel(int k) { g_force_kernel = k; }
        ~ForceKernel() { g_force_kernel = 0; }
    } force_guard(force_kernel);
    // no second pass here: the caller asks for exactly one DP per pair
    mpn_map_opt o2 = *opt;
    o2.zdrop = 0x3fffffff;
    DevRound dv;
    if (tl_slot->pool_jobs.ensure((size_t)n * sizeof(ExtJob) + 16)) return -1;
    MPN_HIP_CHECK(hipMemcpy(tl_slot->pool_jobs.p, jobs.data(), (size_t)n * sizeof(ExtJob), hipMemcpyHostToDevice));
    {
        const unsigned long long cnt = (unsigned long long)n;
        if (tl_slot->pool_used.ensure(128)) return -1;
        MPN_HIP_CHECK(hipMemcpy(tl_slot->pool_used.as<unsigned long long>() + 3, &cnt, 8, hipMemcpyHostToDevice));
    }
    StreamLease sl(st);
    const int rc = run_jobs(in.rv, &o2, n, in.d_reads.p, in.d_qoff.p, in.d_qlen.p, dv, nullptr, sl);
    if (rc) return rc;
    // (the product keeps these on the device for the stitching kernel; the stage test reads them back)
    std::vector<ExtRes> res((size_t)n);
    unsigned long long h_used = 0;
    MPN_HIP_CHECK(hipMemcpy(res.data(), dv.res, (size_t)n * sizeof(ExtRes), hipMemcpyDeviceToHost));
    MPN_HIP_CHECK(hipMemcpy(&h_used, dv.used, 8, hipMemcpyDeviceToHost));
    std::vector<uint32_t> cig((size_t)h_used + 1);
    if (h_used) MPN_HIP_CHECK(hipMemcpy(cig.data(), dv.compact, (size_t)h_used * 4, hipMemcpyDeviceToHost));
    int64_t used = 0;
    for (int i = 0; i < n; ++i) {
        const ExtRes &e = res[i];
        int32_t *o = out9 + (size_t)i * 9;
        o[0] = e.max; o[1] = e.zdropped; o[2] = e.max_q; o[3] = e.max_t; o[4] = e.mqe; o[5] = e.mqe_t; o[6] = e.score; o[7] = e.reach_end;
        o[8] = e.n_cigar;
        cig_off[i] = used;
        if (used + e.n_cigar > cigar_cap) return -3;
        if (e.n_cigar) memcpy(cigar_pool + used, cig.data() + e.cig_pos, (size_t)e.n_cigar * 4);
        used += e.n_cigar;
    }
    return 0;
}

// stage entry point for the tests of the difference-string kernel: aln_tags_wave_kernel, as the product launches it, on
// arbitrary (read, target, CIGAR) triples
extern "C" int mpn_aln_tags_batch(int32_t n, const uint8_t *qcodes, const int64_t *q_off, const int32_t *q_len, const int32_t *qs,
                                  const int32_t *qe, const int32_t *rev, const uint8_t *tcodes, const int64_t *t_off, const int32_t *t_len,
                                  const int32_t *ts, const uint32_t *cigar, const int64_t *cig_off, const int32_t *n_cigar, int32_t out_tags,
                                  char *cs, int64_t cs_cap, int64_t *cs_off, char *md, int64_t md_cap, int64_t *md_off, uint32_t *eqx,
                                  int64_t eqx_cap, int64_t *eqx_off) {
    std::lock_guard<std::mutex> call_guard(g_call_mu);
    hipStream_t st = 0;
    if (n < 0) { set_error("mpn_aln_tags_batch: negative count"); return -1; }
    if (cs_off) cs_off[0] = 0;
    if (md_off) md_off[0] = 0;
    if (eqx_off) eqx_off[0] = 0;
    if (n == 0) return 0;
    const int tags = norm_tags(out_tags);
    if (((tags & MPN_TAG_CS) && !cs_off) || ((tags & MPN_TAG_MD) && !md_off) || ((tags & MPN_TAG_EQX) && !eqx_off)) { set_error("mpn_aln_tags_batch: an output that out_tags asks for has no offset array"); return -1; }
    // everything is checked before any launch: only M/I/D ops, none empty, exactly the read interval, inside the target
    StagePairsDev in;
    if (in.upload_alns("mpn_aln_tags_batch", n, qcodes, q_off, q_len, qs, qe, rev, tcodes, t_off, t_len, ts, cigar, cig_off, n_cigar, false, st)) return -1;
    std::vector<FinOut> fouts((size_t)n, FinOut{});
    for (int i = 0; i < n; ++i) fouts[(size_t)i].n_cigar = n_cigar[i];
    DevBuf<FinOut> d_fo;
    if (d_fo.upload(fouts.data(), fouts.size(), st)) return -1;
    Slot &SL = *tl_slot;
    TagRun tr;
    if (tags_enqueue(SL, in.dims, n, in.sp.ctot, in.d_fj.p, d_fo.p, in.d_cig.p, in.d_reads.p, in.d_qoff.p, in.d_qlen.p, in.rv, tags, st, tr)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (tags_fetch(SL, tr, st)) return -1;
    int64_t c_used = 0, m_used = 0, e_used = 0;
    for (int i = 0; i < n; ++i) {
        const TagOut &to = tr.h_out[i];
        if (tags & MPN_TAG_CS) {
            if (c_used + to.cs_len > cs_cap) return -3;
            if (to.cs_len) memcpy(cs + c_used, tr.h_cs + to.cs_off, (size_t)to.cs_len);
            c_used += to.cs_len; cs_off[i + 1] = c_used;
        }
        if (tags & MPN_TAG_MD) {
            if (m_used + to.md_len > md_cap) return -3;
            if (to.md_len) memcpy(md + m_used, tr.h_md + to.md_off, (size_t)to.md_len);
            m_used += to.md_len; md_off[i + 1] = m_used;
        }
        if (tags & MPN_TAG_EQX) {
            if (e_used + to.n_eqx > eqx_cap) return -3;
            if (to.n_eqx) memcpy(eqx + e_used, tr.h_eqx + to.eqx_off, (size_t)to.n_eqx * 4);
            e_used += to.n_eqx; eqx_off[i + 1] = e_used;
        }
    }
    return 0;
}

// stage entry point for the tests of the finishing kernel: aln_finish_wave_kernel, launched by fin_enqueue as the product
// launches it, on arbitrary (read, target, CIGAR) triples
extern "C" int mpn_aln_finish_batch(const mpn_map_opt *opt, int32_t n, const uint8_t *qcodes, const int64_t *q_off, const int32_t *q_len,
                                    const int32_t *qs, const int32_t *qe, const int32_t *rev, const uint8_t *tcodes, const int64_t *t_off,
                                    const int32_t *t_len, const int32_t *ts, const uint32_t *cigar, const int64_t *cig_off, const int32_t *n_cigar,
                                    int32_t force_class, int32_t *out8, uint32_t *cigar_out) {
    std::lock_guard<std::mutex> call_guard(g_call_mu);
    hipStream_t st = 0;
    if (n < 0) { set_error("mpn_aln_finish_batch: negative count"); return -1; }
    if (n == 0) return 0;
    if (!opt || !out8 || !cigar_out) { set_error("mpn_aln_finish_batch: options or an output array missing"); return -1; }
    // everything is checked before any launch: only M/I/D ops (empty ones allowed), exactly the read interval, inside the target
    StagePairsDev in;
    if (in.upload_alns("mpn_aln_finish_batch", n, qcodes, q_off, q_len, qs, qe, rev, tcodes, t_off, t_len, ts, cigar, cig_off, n_cigar, true, st)) return -1;
    std::vector<FinOut> fouts((size_t)n, FinOut{});
    DevBuf<FinOut> d_fo;
    if (d_fo.upload(fouts.data(), fouts.size(), st)) return -1;
    FinRun fr;
    if (fin_enqueue(in.dims, in.sp.ctot, opt, in.d_fj.p, d_fo.p, in.d_cig.p, in.d_reads.p, in.d_qoff.p, in.d_qlen.p, in.rv, force_class, st, fr)) return -1;
    if (d_fo.download(fouts.data(), fouts.size(), st) || in.d_cig.download(in.sp.cigar.data(), (size_t)in.sp.ctot, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        const FinOut &f = fouts[(size_t)i];
        if (f.n_cigar < 0 || f.n_cigar > n_cigar[i]) { set_error("mpn_aln_finish_batch: pair %d: the kernel returned %d ops for a CIGAR of %d", i, f.n_cigar, n_cigar[i]); return -1; }
        int32_t *o = out8 + (size_t)i * 8;
        o[0] = f.n_cigar; o[1] = f.qshift; o[2] = f.tshift; o[3] = f.blen; o[4] = f.mlen; o[5] = f.n_ambi; o[6] = f.dp_max; o[7] = f.pad;
        if (f.n_cigar) memcpy(cigar_out + cig_off[i], in.sp.cigar.data() + cig_off[i], (size_t)f.n_cigar * 4);
    }
    return 0;
}

// stage entry point for the tests of the hit stage: hit_select_kernel, the host functions and anchor_squeeze_kernel, run by
// hits_from_chains as the mapper runs them, on arbitrary chains.  Arrays are CSR over reads; chains and anchors in pool order
// (chain c's anchors follow those of chains 0..c-1 of its read).  hits: 15 words per hit, in hit order: fx, fy, lx, ly, score,
// score0, cnt, as, parent, subsc, n_sub, mlen, blen, hash, sam_pri; room for one hit per chain.  sq_anchors (with opt->with_cigar):
// the squeezed lists as (x, y) pairs, read after read; room for every anchor.
extern "C" int mpn_hit_select_batch(const mpn_map_opt *opt, int32_t k, int32_t n, const int32_t *q_len, const char *const *names,
                                    const int64_t *chain_off, const uint64_t *u, const uint64_t *fx, const uint64_t *fy, const uint64_t *lx,
                                    const uint64_t *ly, const int32_t *mlen, const int32_t *blen, const int64_t *anchor_off, const uint64_t *anchors,
                                    int32_t path, int32_t max_chains, int32_t grid_cap, int32_t *n_regs, int32_t *n_a, int64_t *hits,
                                    uint64_t *sq_anchors) {
    std::lock_guard<std::mutex> call_guard(g_call_mu);
    if (n < 0) { set_error("mpn_hit_select_batch: negative count"); return -1; }
    if (n == 0) return 0;
    if (!opt || !q_len || !chain_off || !anchor_off || !n_regs || !n_a || !hits || (opt->with_cigar && !sq_anchors)) {
        set_error("mpn_hit_select_batch: options or an array missing"); return -1;
    }
    if (path < 0 || path > 2 || max_chains < 0 || max_chains > HIT_MAX_CHAINS || grid_cap < 0 || k < 1) {
        set_error("mpn_hit_select_batch: path, max_chains, grid_cap or k out of range"); return -1;
    }
    // everything is checked here, before any launch
    if (!stage_csr_ok("mpn_hit_select_batch", n, chain_off, set_error) || !stage_csr_ok("mpn_hit_select_batch", n, anchor_off, set_error)) return -1;
    for (int i = 0; i < n; ++i)
        if (q_len[i] <= 0) { set_error("mpn_hit_select_batch: read %d: no length", i); return -1; }
    const int64_t n_chains = chain_off[n], n_anch = anchor_off[n];
    if (n_chains > 0 && (!u || !fx || !fy || !lx || !ly || !mlen || !blen || !anchors)) { set_error("mpn_hit_select_batch: a chain array missing"); return -1; }
    std::vector<ChainRec> recs((size_t)n_chains + 1);
    {
        std::vector<uint64_t> firsts;
        for (int i = 0; i < n; ++i) {
            int64_t a = anchor_off[i];
            firsts.clear();
            for (int64_t c = chain_off[i]; c < chain_off[i + 1]; ++c) {
                const int32_t cnt = (int32_t)u[c];
                if (cnt < 1 || a + cnt > anchor_off[i + 1]) { set_error("mpn_hit_select_batch: read %d: a chain without anchors, or more than the read has", i); return -1; }
                const uint64_t *f = anchors + 2 * a, *l = anchors + 2 * (a + cnt - 1);
                if (fx[c] != f[0] || fy[c] != f[1] || lx[c] != l[0] || ly[c] != l[1]) {
                    set_error("mpn_hit_select_batch: read %d: a chain record differs from its first or last anchor", i); return -1;
                }
                recs[(size_t)c] = ChainRec{fx[c], fy[c], lx[c], ly[c], mlen[c], blen[c]};
                firsts.push_back(fx[c]);
                a += cnt;
            }
            if (a != anchor_off[i + 1]) { set_error("mpn_hit_select_batch: read %d: the chains' counts do not add up to its anchors", i); return -1; }
            std::sort(firsts.begin(), firsts.end());
            if (std::adjacent_find(firsts.begin(), firsts.end()) != firsts.end()) { set_error("mpn_hit_select_batch: read %d: two chains start at the same anchor", i); return -1; }
        }
    }
    HostChains h;
    h.n_chain.resize((size_t)n); h.u_pos.resize((size_t)n); h.b_pos.resize((size_t)n); h.rep_len.assign((size_t)n, 0);
    h.chain_off.assign(chain_off, chain_off + n + 1);
    std::vector<uint32_t> name_hash((size_t)n);
    for (int i = 0; i < n; ++i) {
        h.n_chain[(size_t)i] = (int32_t)(chain_off[i + 1] - chain_off[i]); h.u_pos[(size_t)i] = chain_off[i]; h.b_pos[(size_t)i] = anchor_off[i];
        name_hash[(size_t)i] = names && names[i] ? x31_hash(names[i]) : 0;
    }
    const uint64_t u_none = 0;
    h.u_all = n_chains ? u : &u_none; h.rec_all = recs.data(); h.n_pool_chains = n_chains;
    StreamLease st((hipStream_t)0);
    DevBuf<int32_t> d_n_chain, d_len;
    DevBuf<int64_t> d_u_pos, d_b_pos;
    DevBuf<uint64_t> d_u;
    DevBuf<ChainRec> d_recs;
    DevBuf<u128> d_chained;
    DevBuf<uint32_t> d_name_hash;
    if (d_n_chain.upload(h.n_chain.data(), (size_t)n, st) || d_len.upload(q_len, (size_t)n, st) || d_u_pos.upload(h.u_pos.data(), (size_t)n, st) ||
        d_b_pos.upload(h.b_pos.data(), (size_t)n, st) || d_u.upload(h.u_all, (size_t)std::max<int64_t>(1, n_chains), st) ||
        d_recs.upload(recs.data(), recs.size(), st) || d_chained.upload(reinterpret_cast<const u128 *>(n_anch ? anchors : &u_none), (size_t)n_anch, st) ||
        d_name_hash.upload(name_hash.data(), (size_t)n, st))
        return -1;
    std::vector<ReadState> rs((size_t)n);
    HitStageBufs hb;
    int64_t *sq_off = nullptr;
    WallTimer wt;
    const HitChainsDev dc{d_n_chain.p, d_u_pos.p, d_b_pos.p, d_u.p, d_recs.p, d_chained.p};
    if (hits_from_chains(opt, k, n, dc, h, nullptr, q_len, d_len.p, d_name_hash.p, names, path, max_chains ? max_chains : HIT_MAX_CHAINS, grid_cap, 1, st,
                         rs.data(), hb, sq_off, wt))
        return -1;
    if (sq_off[n] > n_anch) { set_error("mpn_hit_select_batch: the squeezed lists hold more anchors than the reads have"); return -1; }
    if (opt->with_cigar && sq_off[n] > 0) MPN_HIP_CHECK(hipMemcpyAsync(sq_anchors, hb.a.p, (size_t)sq_off[n] * sizeof(u128), hipMemcpyDeviceToHost, st));
    MPN_HIP_CHECK(stream_sync(st));
    int64_t w = 0;
    for (int i = 0; i < n; ++i) {
        const ReadState &S = rs[(size_t)i];
        if ((int64_t)S.regs.size() > chain_off[i + 1] - chain_off[i]) { set_error("mpn_hit_select_batch: read %d: more hits than chains", i); return -1; }
        n_regs[i] = (int32_t)S.regs.size(); n_a[i] = S.n_a;
        for (const Reg &r : S.regs) {
            int64_t *o = hits + 15 * w++;
            o[0] = (int64_t)r.fx; o[1] = (int64_t)r.fy; o[2] = (int64_t)r.lx; o[3] = (int64_t)r.ly; o[4] = r.score; o[5] = r.score0; o[6] = r.cnt; o[7] = r.as;
            o[8] = r.parent; o[9] = r.subsc; o[10] = r.n_sub; o[11] = r.mlen; o[12] = r.blen; o[13] = (int64_t)r.hash; o[14] = (int64_t)r.sam_pri;
        }
    }
    return 0;
}

// stage entry point for the tests of the extension planning stage: plan_kernel, launched by plan_enqueue as the mapper's round loop
// launches it, on arbitrary hits of arbitrary squeezed anchor lists.  Arrays are CSR over reads (anchors, hits).  hits_out: 11
// words per hit in input order: n_jobs, as1, cnt1, qs, rs, qe, re, qs0, qe0, rid, rev.  win_out: 13 words per window: read, rid, rev,
// qs, qlen, ts, tlen, reversed, w, zdrop, end_bonus, flag, job_anchor; the windows of hit 0, then those of hit 1, ... (the kernel
// places the hits' window groups in no particular order: they are put in hit order here, by first_job).
extern "C" int mpn_ext_plan_batch(const mpn_map_opt *opt, int32_t k, int32_t n_targets, const int32_t *t_len, int32_t n, const int32_t *q_len,
                                  const int64_t *anchor_off, const uint64_t *anchors, const int64_t *hit_off, const int32_t *h_as,
                                  const int32_t *h_cnt, const int32_t *h_mlen, const int32_t *h_split_inv, int32_t grid_cap,
                                  int32_t *hits_out, int64_t win_cap, int64_t *n_win, int32_t *win_out, uint64_t *anchors_out) {
    std::lock_guard<std::mutex> call_guard(g_call_mu);
    hipStream_t st = 0;
    if (n < 0) { set_error("mpn_ext_plan_batch: negative count"); return -1; }
    if (n_win) *n_win = 0;
    if (n == 0) return 0;
    if (!opt || !t_len || !q_len || !anchor_off || !hit_off || !hits_out || !n_win || !win_out || !anchors_out) {
        set_error("mpn_ext_plan_batch: options or an array missing"); return -1;
    }
    if (k < 1 || k > 255 || n_targets < 1 || grid_cap < 0 || win_cap < 0) { set_error("mpn_ext_plan_batch: k, n_targets, grid_cap or win_cap out of range"); return -1; }
    // everything is checked here, before any launch
    if (!stage_csr_ok("mpn_ext_plan_batch", n, anchor_off, set_error) || !stage_csr_ok("mpn_ext_plan_batch", n, hit_off, set_error)) return -1;
    for (int t = 0; t < n_targets; ++t)
        if (t_len[t] <= 0) { set_error("mpn_ext_plan_batch: target %d: no length", t); return -1; }
    for (int i = 0; i < n; ++i)
        if (q_len[i] <= 0) { set_error("mpn_ext_plan_batch: read %d: no length", i); return -1; }
    const int64_t n_anch = anchor_off[n], n_hits64 = hit_off[n];
    if (n_hits64 > 0x3fffffff) { set_error("mpn_ext_plan_batch: too many hits"); return -1; }
    const int n_hits = (int)n_hits64;
    if (n_hits == 0) return 0;
    if (!anchors || !h_as || !h_cnt || !h_mlen || !h_split_inv) { set_error("mpn_ext_plan_batch: a hit array missing"); return -1; }
    std::vector<PlanReg> pregs((size_t)n_hits);
    int64_t cap_need = 0, cap_dev = 0;
    {
        std::vector<std::pair<int32_t, int32_t>> iv;
        for (int i = 0; i < n; ++i) {
            const int64_t n_a = anchor_off[i + 1] - anchor_off[i];
            const uint64_t *a = anchors + 2 * anchor_off[i];
            for (int64_t j = 0; j < n_a; ++j) {   // the walks over a hit's neighbours read every anchor of the read
                const uint64_t x = a[2 * j], y = a[2 * j + 1];
                const int64_t rid = (int64_t)(x << 1 >> 33);
                const int32_t span = (int32_t)(y >> 32 & 0xff);
                if (rid >= n_targets || (int32_t)x < 0 || (int32_t)x >= t_len[rid] || (int32_t)y < 0 || (int32_t)y >= q_len[i] || span < 1 || y >> 43) {
                    set_error("mpn_ext_plan_batch: read %d: anchor %lld outside its target or the read, without span, or with unknown flags", i, (long long)j); return -1;
                }
            }
            iv.clear();
            for (int64_t h = hit_off[i]; h < hit_off[i + 1]; ++h) {
                const int32_t as = h_as[h], cnt = h_cnt[h];
                if (cnt < 1 || as < 0 || (int64_t)as + cnt > n_a) { set_error("mpn_ext_plan_batch: read %d: a hit without anchors, or beyond the read's", i); return -1; }
                for (int32_t j = as + 1; j < as + cnt; ++j) {
                    const uint64_t *p = a + 2 * (j - 1), *c = a + 2 * j;
                    if (p[0] >> 32 != c[0] >> 32) { set_error("mpn_ext_plan_batch: read %d: a hit on two targets or strands", i); return -1; }
                    if ((int32_t)c[0] <= (int32_t)p[0] || (int32_t)c[1] <= (int32_t)p[1]) {
                        set_error("mpn_ext_plan_batch: read %d: anchor %d of a hit does not lie behind the one before it", i, j); return -1;
                    }
                }
                iv.push_back({as, as + cnt});
                pregs[(size_t)h] = PlanReg{anchor_off[i], (int32_t)n_a, as, cnt, h_mlen[h], i, q_len[i], h_split_inv[h] ? 1 : 0, 0};
                cap_need += (int64_t)cnt + 1;   // a hit of cnt anchors has at most cnt + 1 windows
                cap_dev += (int64_t)cnt + 2;    // (the room the mapper gives it)
            }
            std::sort(iv.begin(), iv.end());
            for (size_t q = 1; q < iv.size(); ++q)
                if (iv[q].first < iv[q - 1].second) { set_error("mpn_ext_plan_batch: read %d: two hits share an anchor", i); return -1; }
        }
    }
    if (cap_need > win_cap || cap_dev > 0x7fffffff) { set_error("mpn_ext_plan_batch: room for %lld windows needed", (long long)cap_need); return -1; }
    DevBuf<u128> d_a;
    DevBuf<int32_t> d_tl, d_janchor;
    DevBuf<PlanReg> d_pr;
    DevBuf<PlanSum> d_ps;
    DevBuf<StitchReg> d_sr;
    DevBuf<ExtJob> d_jobs;
    DevBuf<unsigned long long> d_used;
    if (d_a.upload(reinterpret_cast<const u128 *>(anchors), (size_t)n_anch, st) || d_tl.upload(t_len, (size_t)n_targets, st) ||
        d_pr.upload(pregs.data(), pregs.size(), st) || d_ps.alloc((size_t)n_hits) || d_sr.alloc((size_t)n_hits) ||
        d_jobs.alloc((size_t)cap_dev) || d_janchor.alloc((size_t)cap_dev) || d_used.alloc(16))
        return -1;
    if (plan_enqueue(opt, k, d_pr.p, n_hits, d_a.p, d_tl.p, d_used.p, d_jobs.p, d_janchor.p, d_sr.p, d_ps.p, grid_cap, st)) return -1;
    std::vector<StitchReg> sregs((size_t)n_hits);
    std::vector<PlanSum> psum((size_t)n_hits);
    unsigned long long used[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (d_sr.download(sregs.data(), sregs.size(), st) || d_ps.download(psum.data(), psum.size(), st) || d_used.download(used, 8, st) ||
        d_a.download(reinterpret_cast<u128 *>(anchors_out), (size_t)n_anch, st))
        return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    const int64_t total = (int64_t)used[3];
    if (total < 0 || total > cap_need) { set_error("mpn_ext_plan_batch: the kernel counted %lld windows, %lld at most expected", (long long)total, (long long)cap_need); return -1; }
    int64_t sum = 0;
    for (int h = 0; h < n_hits; ++h) {
        const StitchReg &s = sregs[(size_t)h];
        if (s.n_jobs < 0 || s.n_jobs > pregs[(size_t)h].cnt + 1 || s.first_job < 0 || (int64_t)s.first_job + s.n_jobs > total) {
            set_error("mpn_ext_plan_batch: hit %d: windows [%d, +%d) of %lld", h, s.first_job, s.n_jobs, (long long)total); return -1;
        }
        sum += s.n_jobs;
    }
    if (sum != total) { set_error("mpn_ext_plan_batch: the hits hold %lld windows, the counter %lld", (long long)sum, (long long)total); return -1; }
    std::vector<ExtJob> jobs((size_t)total + 1);
    std::vector<int32_t> janchor((size_t)total + 1);
    if (total > 0) {
        if (d_jobs.download(jobs.data(), (size_t)total, st) || d_janchor.download(janchor.data(), (size_t)total, st)) return -1;
        MPN_HIP_CHECK(hipStreamSynchronize(st));
    }
    int64_t w = 0;
    for (int h = 0; h < n_hits; ++h) {
        const StitchReg &s = sregs[(size_t)h];
        int32_t *o = hits_out + (size_t)h * 11;
        o[0] = s.n_jobs; o[1] = psum[(size_t)h].as1; o[2] = psum[(size_t)h].cnt1; o[3] = s.qs; o[4] = s.rs; o[5] = s.qe; o[6] = s.re; o[7] = s.qs0;
        o[8] = s.qe0; o[9] = s.rid; o[10] = s.rev;
        for (int j = 0; j < s.n_jobs; ++j, ++w) {
            const ExtJob &jb = jobs[(size_t)s.first_job + j];
            int32_t *q = win_out + (size_t)w * 13;
            q[0] = jb.read; q[1] = jb.rid; q[2] = jb.rev; q[3] = jb.qs; q[4] = jb.qlen; q[5] = jb.ts; q[6] = jb.tlen; q[7] = jb.reversed; q[8] = jb.w;
            q[9] = jb.zdrop; q[10] = jb.end_bonus; q[11] = jb.flag; q[12] = janchor[(size_t)s.first_job + j];
        }
    }
    *n_win = w;
    return 0;
}

// stage entry point for the tests of the stitching stage: stitch_kernel, launched by stitch_enqueue as stitch_and_finish launches
// it, on arbitrary hits, windows, window results and compact-pool contents.  hits: 15 words per hit; wins: 13 words per window;
// out: 25 int64 per hit (StitchOut, then FinJob); splits_out: 8 int64 per cut hit (the SplitRec words, x / y bit for bit).
extern "C" int mpn_stitch_batch(int32_t n, const int64_t *anchor_off, const uint64_t *anchors, int32_t n_hits, const int32_t *hits,
                                int64_t n_win, const int32_t *wins, const int64_t *cig_pos, int64_t n_compact, const uint32_t *compact,
                                int32_t min_cnt, int32_t grid_cap, int64_t *out, int64_t pool_cap, uint32_t *pool_out, int64_t *pool_used,
                                int64_t *splits_out, int64_t *n_splits) {
    std::lock_guard<std::mutex> call_guard(g_call_mu);
    hipStream_t st = 0;
    constexpr int HW = 15, WW = 13;
    constexpr int32_t LIM = 1 << 28, KNOWN = EZ_APPROX_MAX | EZ_RIGHT | EZ_EXTZ_ONLY | EZ_REV_CIGAR | EZ_REFUSED | EZ_INV;
    if (n < 0 || n_hits < 0 || n_win < 0 || n_compact < 0) { set_error("mpn_stitch_batch: negative count"); return -1; }
    if (pool_used) *pool_used = 0;
    if (n_splits) *n_splits = 0;
    if (n_hits == 0) return 0;
    if (!anchor_off || !hits || !out || !pool_used || !n_splits || !splits_out || (n_win > 0 && (!wins || !cig_pos)) || (n_compact > 0 && !compact)) {
        set_error("mpn_stitch_batch: an array missing"); return -1;
    }
    if (min_cnt < 0 || grid_cap < 0 || pool_cap < 0 || n_win > 0x3fffffff || n_compact > 0x3fffffff) {
        set_error("mpn_stitch_batch: min_cnt, grid_cap, pool_cap or a count out of range"); return -1;
    }
    // everything is checked here, before any launch
    if (!stage_csr_ok("mpn_stitch_batch", n, anchor_off, set_error)) return -1;
    const int64_t n_anch = n > 0 ? anchor_off[n] : 0;
    if (n_anch > 0 && !anchors) { set_error("mpn_stitch_batch: an array missing"); return -1; }
    std::vector<StitchReg> sregs((size_t)n_hits);
    std::vector<PlanReg> pregs((size_t)n_hits);
    std::vector<PlanSum> psum((size_t)n_hits);
    std::vector<ExtJob> jobs((size_t)n_win + 1);
    std::vector<ExtRes> res((size_t)n_win + 1);
    std::vector<int32_t> janchor((size_t)n_win + 1);
    int64_t ops_max = 0;
    {
        std::vector<std::pair<int64_t, int64_t>> wiv, civ;
        auto coord = [](int32_t v) { return v >= -LIM && v <= LIM; };
        for (int h = 0; h < n_hits; ++h) {
            const int32_t *q = hits + (size_t)h * HW;
            const int32_t read = q[0], rid = q[1], rev = q[2], as = q[3], cnt = q[4], as1 = q[5], cnt1 = q[6], first = q[13], nj = q[14];
            if (read < 0 || read >= n) { set_error("mpn_stitch_batch: hit %d: no such read", h); return -1; }
            const int64_t n_a = anchor_off[read + 1] - anchor_off[read];
            if (rid < 0 || (rev != 0 && rev != 1)) { set_error("mpn_stitch_batch: hit %d: target or strand out of range", h); return -1; }
            if (as < 0 || cnt < 1 || (int64_t)as + cnt > n_a || as1 < as || cnt1 < 1 || (int64_t)as1 + cnt1 > (int64_t)as + cnt) {
                set_error("mpn_stitch_batch: hit %d: anchors [%d, +%d) trimmed to [%d, +%d) of %lld", h, as, cnt, as1, cnt1, (long long)n_a); return -1;
            }
            for (int c = 7; c < 13; ++c)
                if (!coord(q[c])) { set_error("mpn_stitch_batch: hit %d: a coordinate out of range", h); return -1; }
            if (nj < 0 || first < 0 || (int64_t)first + nj > n_win) { set_error("mpn_stitch_batch: hit %d: windows [%d, +%d) of %lld", h, first, nj, (long long)n_win); return -1; }
            if (nj > 0) wiv.push_back({first, (int64_t)first + nj});
            int64_t op_len = 0;
            for (int k = 0; k < nj; ++k) {
                const int64_t wi = (int64_t)first + k;
                const int32_t *w = wins + (size_t)wi * WW;
                const int32_t flag = w[0], reversed = w[1], anchor = w[4], zdropped = w[6], reach_end = w[11], nc = w[12];
                if ((flag & ~KNOWN) || (reversed != 0 && reversed != 1) || !coord(w[2]) || !coord(w[3])) {
                    set_error("mpn_stitch_batch: hit %d: window %d: unknown flags, or a coordinate out of range", h, k); return -1;
                }
                if (flag & EZ_EXTZ_ONLY) {   // an end extension: the left one first, the right one last
                    if (anchor != -1 || (flag & EZ_INV) || (reversed ? k != 0 : k != nj - 1)) {
                        set_error("mpn_stitch_batch: hit %d: window %d: an extension out of place, with an anchor or with the inversion mark", h, k); return -1;
                    }
                } else if (reversed || anchor < 1 || anchor > cnt1 - 1 || (flag & (EZ_INV | EZ_REFUSED)) == (EZ_INV | EZ_REFUSED)) {
                    set_error("mpn_stitch_batch: hit %d: window %d: a fill read backwards, without an anchor of the hit to end at, or refused and tested", h, k); return -1;
                }
                ExtJob jb;
                memset(&jb, 0, sizeof(jb));
                jb.read = read; jb.rid = rid; jb.rev = rev; jb.qs = w[2]; jb.ts = w[3]; jb.reversed = reversed; jb.flag = flag; jb.cls = -1;
                jobs[(size_t)wi] = jb;
                janchor[(size_t)wi] = anchor;
                ExtRes e;
                memset(&e, 0, sizeof(e));
                e.max = w[5]; e.zdropped = zdropped; e.max_q = w[7]; e.max_t = w[8]; e.mqe_t = w[9]; e.mqe = 0; e.score = w[10]; e.reach_end = reach_end;
                e.n_cigar = nc; e.cig_pos = cig_pos[wi];
                res[(size_t)wi] = e;
                if (flag & EZ_REFUSED) continue;   // (a placeholder's result record is never read)
                if ((zdropped != 0 && zdropped != 1) || (reach_end != 0 && reach_end != 1) || !coord(e.max) || !coord(e.score) || e.max_q < -1 || e.max_q > LIM ||
                    e.max_t < -1 || e.max_t > LIM || e.mqe_t < -1 || e.mqe_t > LIM) {
                    set_error("mpn_stitch_batch: hit %d: window %d: a result out of range", h, k); return -1;
                }
                if (nc < 0 || e.cig_pos < 0 || e.cig_pos + nc > n_compact) { set_error("mpn_stitch_batch: hit %d: window %d: operations outside the pool", h, k); return -1; }
                if (nc > 0) civ.push_back({e.cig_pos, e.cig_pos + nc});
                for (int32_t c = 0; c < nc; ++c) {
                    const uint32_t op = compact[e.cig_pos + c];
                    if ((op & 0xf) > 2) { set_error("mpn_stitch_batch: hit %d: window %d: operation %d is not M, I or D", h, k, c); return -1; }
                    op_len += op >> 4;
                }
                ops_max += nc;
            }
            // (merged operations are added up in place: no run of them may reach the kind bits' neighbour, bit 32)
            if (op_len >= LIM) { set_error("mpn_stitch_batch: hit %d: operations of 2^28 bases or more", h); return -1; }
            sregs[(size_t)h] = StitchReg{first, nj, q[7], q[8], q[9], q[10], q[11], q[12], read, rid, rev, 0};
            pregs[(size_t)h] = PlanReg{anchor_off[read], (int32_t)n_a, as, cnt, 0, read, 0, 0, 0};
            psum[(size_t)h] = PlanSum{as1, cnt1};
        }
        for (auto *iv : {&wiv, &civ}) {
            std::sort(iv->begin(), iv->end());
            for (size_t q = 1; q < iv->size(); ++q)
                if ((*iv)[q].first < (*iv)[q - 1].second) {
                    set_error(iv == &wiv ? "mpn_stitch_batch: two hits share a window" : "mpn_stitch_batch: two windows share operations of the pool"); return -1;
                }
        }
    }
    if (ops_max > pool_cap) { set_error("mpn_stitch_batch: room for %lld operations needed", (long long)ops_max); return -1; }
    if (ops_max > 0 && !pool_out) { set_error("mpn_stitch_batch: an array missing"); return -1; }
    DevBuf<u128> d_a;
    DevBuf<int32_t> d_janchor;
    DevBuf<PlanReg> d_pr;
    DevBuf<PlanSum> d_ps;
    DevBuf<StitchReg> d_sr;
    DevBuf<ExtJob> d_jobs;
    DevBuf<ExtRes> d_res;
    DevBuf<uint32_t> d_compact, d_cig;
    DevBuf<StitchOut> d_so;
    DevBuf<FinJob> d_fj;
    DevBuf<SplitRec> d_splits;
    DevBuf<unsigned long long> d_used;
    if (d_a.upload(reinterpret_cast<const u128 *>(anchors), (size_t)n_anch, st) || d_pr.upload(pregs.data(), pregs.size(), st) ||
        d_ps.upload(psum.data(), psum.size(), st) || d_sr.upload(sregs.data(), sregs.size(), st) || d_jobs.upload(jobs.data(), (size_t)n_win, st) ||
        d_res.upload(res.data(), (size_t)n_win, st) || d_janchor.upload(janchor.data(), (size_t)n_win, st) ||
        d_compact.upload(compact, (size_t)n_compact, st) || d_cig.alloc((size_t)pool_cap) || d_so.alloc((size_t)n_hits) || d_fj.alloc((size_t)n_hits) ||
        d_splits.alloc((size_t)n_hits) || d_used.alloc(8))
        return -1;
    MPN_HIP_CHECK(hipMemsetAsync(d_used.p, 0, 64, st));   // the counter block of a round: [2] stitched ops, [6] cut hits
    const RoundDev rd{d_sr.p, d_pr.p, d_ps.p, d_janchor.p, d_a.p};
    if (stitch_enqueue(rd, n_hits, d_jobs.p, d_res.p, d_compact.p, d_cig.p, d_used.p + 2, d_so.p, d_fj.p, min_cnt, d_splits.p, d_used.p + 6, grid_cap, st))
        return -1;
    std::vector<StitchOut> so((size_t)n_hits);
    std::vector<FinJob> fj((size_t)n_hits);
    unsigned long long used[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (d_so.download(so.data(), so.size(), st) || d_fj.download(fj.data(), fj.size(), st) || d_used.download(used, 8, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (used[2] > (unsigned long long)ops_max || used[6] > (unsigned long long)n_hits) {
        set_error("mpn_stitch_batch: the kernel counted %llu operations and %llu cut hits, %lld and %d at most expected", used[2], used[6], (long long)ops_max, n_hits);
        return -1;
    }
    std::vector<SplitRec> sp((size_t)used[6] + 1);
    if (d_cig.download(pool_out, (size_t)used[2], st) || d_splits.download(sp.data(), (size_t)used[6], st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    for (int h = 0; h < n_hits; ++h) {
        const StitchOut &o = so[(size_t)h];
        const FinJob &f = fj[(size_t)h];
        int64_t *q = out + (size_t)h * 25;
        q[0] = o.cig_off; q[1] = o.n_ops; q[2] = o.dp_score; q[3] = o.rs1; q[4] = o.re1; q[5] = o.qs1; q[6] = o.qe1; q[7] = o.has_p; q[8] = o.dropped;
        q[9] = o.drop_fill; q[10] = o.drop_max_t; q[11] = o.drop_max_q; q[12] = o.split_n; q[13] = o.split_inv; q[14] = o.split_rec;
        q[15] = f.cig_off; q[16] = f.code_off; q[17] = f.n_cigar; q[18] = f.read; q[19] = f.rid; q[20] = f.rev; q[21] = f.qs1; q[22] = f.rs1;
        q[23] = f.qspan; q[24] = f.tspan;
    }
    for (size_t i = 0; i < (size_t)used[6]; ++i) {
        const SplitRec &r = sp[i];
        int64_t *q = splits_out + i * 8;
        q[0] = (int64_t)r.fx; q[1] = (int64_t)r.fy; q[2] = (int64_t)r.lx_left; q[3] = (int64_t)r.ly_left; q[4] = r.mlen_l; q[5] = r.blen_l; q[6] = r.mlen_r;
        q[7] = r.blen_r;
    }
    *pool_used = (int64_t)used[2];
    *n_splits = (int64_t)used[6];
    return 0;
}
