// Per-read hit bookkeeping of the mapper on the host (hit_host.h): minimap2's hit.c restated on the chain records.  The reads
// with more chains than hit_select_kernel stages take this path from the start; every read takes it after the alignment
// rounds (filter, rank, group, MAPQ) and in the merge of a split index' parts.
#include "hit_host.h"

#include <algorithm>
#include <math.h>

namespace mpn {

thread_local HitScratch tl_hs;

void gen_regs(uint32_t hash, int qlen, int n_u, const ChainIn *c, std::vector<Reg> &regs) {
    struct Z { uint64_t x, y; int i; };
    static thread_local std::vector<Z> z;
    z.resize((size_t)n_u);
    int k = 0;
    for (int i = 0; i < n_u; ++i) {
        const uint32_t h = (uint32_t)hash64((hash64(c[i].rec->fx) + hash64(c[i].rec->fy)) ^ hash);
        z[i].x = c[i].u ^ h;
        z[i].y = (uint64_t)k << 32 | (uint32_t)(int32_t)c[i].u;
        z[i].i = i;
        k += (int32_t)c[i].u;
    }
    std::sort(z.begin(), z.end(), [](const Z &p, const Z &q) { return p.x != q.x ? p.x < q.x : p.y < q.y; });
    regs.assign(n_u, Reg());
    for (int i = 0; i < n_u; ++i) {
        Reg &ri = regs[i];
        const Z &zi = z[n_u - 1 - i];
        const ChainRec &rc = *c[zi.i].rec;
        ri.id = i;
        ri.parent = PARENT_UNSET;
        ri.score = ri.score0 = (int32_t)(zi.x >> 32);
        ri.hash = (uint32_t)zi.x;
        ri.cnt = (int32_t)zi.y;
        ri.as = (int32_t)(zi.y >> 32);
        ri.fx = rc.fx; ri.fy = rc.fy; ri.lx = rc.lx; ri.ly = rc.ly; ri.src = c[zi.i].src;
        ri.mlen = rc.mlen; ri.blen = rc.blen;
        reg_set_coor(ri, qlen);
    }
}

void set_parent(float mask_level, std::vector<Reg> &r, int sub_diff) {
    const int n = (int)r.size();
    if (n <= 0) return;
    for (int i = 0; i < n; ++i) r[i].id = i;
    std::vector<uint64_t> &cov = tl_hs.cov;
    std::vector<int> &w = tl_hs.w;
    if ((int)cov.size() < n) { cov.resize((size_t)n); w.resize((size_t)n); }
    w[0] = 0; r[0].parent = 0;
    int k = 1;
    for (int i = 1; i < n; ++i) {
        Reg &ri = r[i];
        const int si = ri.qs, ei = ri.qe;
        int n_cov = 0, uncov_len = 0, j;
        for (j = 0; j < k; ++j) {
            const Reg &rp = r[w[j]];
            int sj = rp.qs, ej = rp.qe;
            if (ej <= si || sj >= ei) continue;
            if (sj < si) sj = si;
            if (ej > ei) ej = ei;
            cov[n_cov++] = (uint64_t)sj << 32 | (uint32_t)ej;
        }
        if (n_cov > 0) {
            int x = si;
            std::sort(cov.begin(), cov.begin() + n_cov);
            for (j = 0; j < n_cov; ++j) {
                if ((int)(cov[j] >> 32) > x) uncov_len += (int)(cov[j] >> 32) - x;
                x = (int32_t)cov[j] > x ? (int32_t)cov[j] : x;
            }
            if (ei > x) uncov_len += ei - x;
            for (j = 0; j < k; ++j) {
                Reg &rp = r[w[j]];
                const int sj = rp.qs, ej = rp.qe;
                if (ej <= si || sj >= ei) continue;
                const int min = ej - sj < ei - si ? ej - sj : ei - si, max = ej - sj > ei - si ? ej - sj : ei - si;
                const int ol = si < sj ? (ei < sj ? 0 : ei < ej ? ei - sj : ej - sj) : (ej < si ? 0 : ej < ei ? ej - si : ei - si);
                if ((float)ol / min - (float)uncov_len / max > mask_level) {
                    int cnt_sub = 0;
                    ri.parent = rp.parent;
                    rp.subsc = rp.subsc > ri.score ? rp.subsc : ri.score;
                    if (ri.cnt >= rp.cnt) cnt_sub = 1;
                    if (rp.has_p && ri.has_p && (rp.rid != ri.rid || rp.rs != ri.rs || rp.re != ri.re || ol != min)) {
                        rp.dp_max2 = rp.dp_max2 > ri.dp_max ? rp.dp_max2 : ri.dp_max;
                        if (rp.dp_max - ri.dp_max <= sub_diff) cnt_sub = 1;
                    }
                    if (cnt_sub) ++rp.n_sub;
                    break;
                }
            }
        } else j = k;
        if (j == k) { w[k++] = i; ri.parent = i; ri.n_sub = 0; }
    }
}

static void sync_regs(std::vector<Reg> &regs) {
    const int n_regs = (int)regs.size();
    if (n_regs <= 0) return;
    int max_id = -1;
    for (auto &r : regs) max_id = max_id > r.id ? max_id : r.id;
    std::vector<int> tmp(max_id + 1 > 0 ? max_id + 1 : 1, -1);
    for (int i = 0; i < n_regs; ++i) if (regs[i].id >= 0) tmp[regs[i].id] = i;
    for (int i = 0; i < n_regs; ++i) {
        Reg &r = regs[i];
        r.id = i;
        if (r.parent == PARENT_TMP_PRI) r.parent = i;
        else if (r.parent >= 0 && r.parent <= max_id && tmp[r.parent] >= 0) r.parent = tmp[r.parent];
        else r.parent = PARENT_UNSET;
    }
    set_sam_pri(regs);
}

void select_sub(float pri_ratio, int min_diff, int best_n, std::vector<Reg> &r) {
    if (pri_ratio > 0.0f && !r.empty()) {
        const int n = (int)r.size();
        int k = 0, n_2nd = 0;
        for (int i = 0; i < n; ++i) {
            const int p = r[i].parent;
            if (p == i || r[i].inv) { if (k != i) r[k] = r[i]; ++k; }
            else if ((r[i].score >= r[p].score * pri_ratio || r[i].score + min_diff >= r[p].score) && n_2nd < best_n) {
                if (!(r[i].qs == r[p].qs && r[i].qe == r[p].qe && r[i].rid == r[p].rid && r[i].rs == r[p].rs && r[i].re == r[p].re)) {
                    if (k != i) r[k] = r[i];
                    ++k; ++n_2nd;
                }
            }
        }
        // NB: r[p] above may already have been overwritten when p > k; minimap2 has the same in-place semantics
        if (k != n) { r.resize(k); sync_regs(r); }
    }
}

void filter_regs(const mpn_map_opt *opt, int qlen, std::vector<Reg> &regs) {
    int k = 0;
    for (int i = 0; i < (int)regs.size(); ++i) {
        Reg &r = regs[i];
        int flt = 0;
        if (!r.inv && r.cnt < opt->min_cnt) flt = 1;
        if (r.has_p) {
            if (r.mlen < opt->min_chain_score) flt = 1;
            else if (r.dp_max < opt->min_dp_max) flt = 1;
            else if (r.qs > qlen * opt->max_clip_ratio && qlen - r.qe > qlen * opt->max_clip_ratio) flt = 1;
        }
        if (!flt) { if (k < i) regs[k] = regs[i]; ++k; }
    }
    regs.resize(k);
}

int squeeze_a(std::vector<Reg> &regs, int read, int64_t pool_base, std::vector<SqueezeSeg> &segs) {
    const int n_regs = (int)regs.size();
    std::vector<std::pair<uint64_t, int>> &aux = tl_hs.aux;
    aux.resize((size_t)n_regs);
    for (int i = 0; i < n_regs; ++i) aux[i] = {(uint64_t)regs[i].as, i};
    if (n_regs > 1) std::sort(aux.begin(), aux.end());
    int as = 0;
    for (int i = 0; i < n_regs; ++i) {
        Reg &r = regs[aux[i].second];
        r.as = as;
        r.seg = (int32_t)segs.size();
        segs.push_back(SqueezeSeg{pool_base + r.src, as, r.cnt, read, 0});
        as += r.cnt;
    }
    return as;
}

void join_long(const mpn_map_opt *opt, int qlen, std::vector<Reg> &regs, std::vector<SqueezeSeg> &segs) {
    const int n_regs = (int)regs.size();
    if (n_regs < 2) return;
    std::vector<std::pair<uint64_t, int>> &aux = tl_hs.aux;
    aux.clear();
    for (int i = 0; i < n_regs; ++i)
        if (regs[i].parent == i || regs[i].parent < 0) aux.push_back({(uint64_t)regs[i].as, i});
    std::sort(aux.begin(), aux.end());
    int n_drop = 0;
    for (int i = (int)aux.size() - 1; i >= 1; --i) {
        Reg &r0 = regs[aux[i - 1].second], &r1 = regs[aux[i].second];
        if (r0.as + r0.cnt != r1.as) continue;
        if (r0.rid != r1.rid || r0.rev != r1.rev) continue;
        const u128 a0e_{r0.lx, r0.ly}, a1s_{r1.fx, r1.fy};
        const u128 *a0e = &a0e_, *a1s = &a1s_;
        if (a1s->x <= a0e->x || (int32_t)a1s->y <= (int32_t)a0e->y) continue;
        int max_gap, min_gap;
        max_gap = min_gap = (int32_t)a1s->y - (int32_t)a0e->y;
        max_gap = max_gap > (int64_t)(a1s->x - a0e->x) ? max_gap : (int)(a1s->x - a0e->x);
        min_gap = min_gap < (int64_t)(a1s->x - a0e->x) ? min_gap : (int)(a1s->x - a0e->x);
        if (max_gap > opt->max_join_long || min_gap > opt->max_join_short) continue;
        const int sc_thres = (int)((float)opt->min_join_flank_sc / opt->max_join_long * max_gap + .499);
        if (r0.score < sc_thres || r1.score < sc_thres) continue;
        const int min_flank_len = (int)(max_gap * opt->min_join_flank_ratio);
        if (r0.re - r0.rs < min_flank_len || r0.qe - r0.qs < min_flank_len) continue;
        if (r1.re - r1.rs < min_flank_len || r1.qe - r1.qs < min_flank_len) continue;
        segs[(size_t)r1.seg].flag = 1;   // (a[r1.as].y |= SEED_LONG_JOIN, applied by the squeeze kernel)
        r0.cnt += r1.cnt; r0.score += r1.score;
        {   // mm_cal_fuzzy_len over the joined anchors: both parts' sums and the step across the joint
            const int span = (int)(a1s->y >> 32 & 0xff);
            const int tl = (int32_t)a1s->x - (int32_t)a0e->x, ql = (int32_t)a1s->y - (int32_t)a0e->y;
            r0.blen += r1.blen - span + (tl > ql ? tl : ql);
            r0.mlen += r1.mlen - span + (tl > span && ql > span ? span : tl < ql ? tl : ql);
        }
        r0.lx = r1.lx; r0.ly = r1.ly;
        reg_set_coor(r0, qlen);
        r1.cnt = 0;
        r1.parent = r0.id;
        ++n_drop;
    }
    if (n_drop > 0) {
        for (auto &r : regs)
            if (r.parent >= 0 && r.id != r.parent)
                if (regs[r.parent].parent >= 0 && regs[r.parent].parent != r.parent) r.parent = regs[r.parent].parent;
        filter_regs(opt, qlen, regs);
        sync_regs(regs);
    }
}

void hit_sort(std::vector<Reg> &r) {
    const int n = (int)r.size();
    if (n <= 1) return;
    std::vector<std::pair<uint64_t, int>> &aux = tl_hs.aux;
    aux.clear();
    for (int i = 0; i < n; ++i)
        if (r[i].inv || r[i].cnt > 0) aux.push_back({(uint64_t)(uint32_t)(r[i].has_p ? r[i].dp_max : r[i].score) << 32 | r[i].hash, i});
    std::sort(aux.begin(), aux.end());
    const int m = (int)aux.size();
    if (m == n) {
        // every hit stays: permute in place along the cycles (a read of a split, strain-rich target set brings a hundred hits
        // to the merge; a second array of them costs an allocation and a construction + destruction per hit)
        std::vector<int> &from = tl_hs.idx;   // the hit that belongs at place k
        from.resize((size_t)n);
        for (int k = 0; k < n; ++k) from[(size_t)k] = aux[(size_t)(n - 1 - k)].second;
        for (int s0 = 0; s0 < n; ++s0) {
            if (from[(size_t)s0] == s0 || from[(size_t)s0] < 0) continue;
            Reg tmp = std::move(r[(size_t)s0]);
            int k = s0;
            for (;;) {
                const int f = from[(size_t)k];
                from[(size_t)k] = -1;
                if (f == s0) { r[(size_t)k] = std::move(tmp); break; }
                r[(size_t)k] = std::move(r[(size_t)f]);
                k = f;
            }
        }
        return;
    }
    std::vector<Reg> t(aux.size());
    for (int i = m - 1; i >= 0; --i) t[(size_t)(m - 1 - i)] = std::move(r[(size_t)aux[i].second]);
    r.swap(t);
}

void set_mapq(std::vector<Reg> &regs, int min_chain_sc, int match_sc, int rep_len) {
    static const float q_coef = 40.0f;
    if (regs.empty()) return;
    int64_t sum_sc = 0;
    for (auto &r : regs) if (r.parent == r.id) sum_sc += r.score;
    const float uniq_ratio = (float)sum_sc / (sum_sc + rep_len);
    for (auto &r : regs) {
        if (r.inv) r.mapq = 0;
        else if (r.parent == r.id) {
            int mapq;
            float pen_s1 = (r.score > 100 ? 1.0f : 0.01f * r.score) * uniq_ratio;
            float pen_cm = r.cnt > 10 ? 1.0f : 0.1f * r.cnt;
            pen_cm = pen_s1 < pen_cm ? pen_s1 : pen_cm;
            const int subsc = r.subsc > min_chain_sc ? r.subsc : min_chain_sc;
            if (r.has_p && r.dp_max2 > 0 && r.dp_max > 0) {
                const float identity = (float)r.mlen / r.blen;
                const float x = (float)r.dp_max2 * subsc / r.dp_max / r.score0;
                mapq = (int)(identity * pen_cm * q_coef * (1.0f - x * x) * logf((float)r.dp_max / match_sc));
                const int mapq_alt = (int)(6.02f * identity * identity * (r.dp_max - r.dp_max2) / match_sc + .499f);
                mapq = mapq < mapq_alt ? mapq : mapq_alt;
            } else {
                const float x = (float)subsc / r.score0;
                if (r.has_p) {
                    const float identity = (float)r.mlen / r.blen;
                    mapq = (int)(identity * pen_cm * q_coef * (1.0f - x) * logf((float)r.dp_max / match_sc));
                } else mapq = (int)(pen_cm * q_coef * (1.0f - x) * logf(r.score));
            }
            mapq -= (int)(4.343f * logf(r.n_sub + 1) + .499f);
            mapq = mapq > 0 ? mapq : 0;
            r.mapq = mapq < 60 ? mapq : 60;
            if (r.has_p && r.dp_max > r.dp_max2 && r.mapq == 0) r.mapq = 1;
        } else r.mapq = 0;
    }
}

static void split_reg(Reg &r, Reg &r2, int n, int qlen, const SplitRec *sp) {
    if (n <= 0 || n >= r.cnt || !sp) return;
    r2 = r;
    r2.id = -1;
    r2.sam_pri = 0;
    r2.has_p = 0; r2.cigar.clear(); r2.cs.clear(); r2.md.clear(); r2.dp_score = r2.dp_max = r2.dp_max2 = r2.n_ambi = 0;
    r2.split_inv = 0;
    r2.aligned = 0;
    r2.cnt = r.cnt - n;
    r2.score = (int32_t)(r.score * ((float)r2.cnt / r.cnt) + .499);
    r2.as = r.as + n;
    if (r.parent == r.id) r2.parent = PARENT_TMP_PRI;
    r2.fx = sp->fx; r2.fy = sp->fy;   // (its last anchor is the hit's)
    r2.mlen = sp->mlen_r; r2.blen = sp->blen_r;
    reg_set_coor(r2, qlen);
    r.cnt -= r2.cnt;
    r.score -= r2.score;
    r.lx = sp->lx_left; r.ly = sp->ly_left;
    r.mlen = sp->mlen_l; r.blen = sp->blen_l;
    reg_set_coor(r, qlen);
    r.split |= 1; r2.split |= 2;
}

bool apply_stitch(int qlen, Reg &r, Reg &r2, const SplitRec *splits, const StitchOut &so, int fin_idx) {
    bool has_r2 = false;
    r2.cnt = 0;
    if (so.has_p) r.has_p = 1;
    r.dp_score += so.dp_score;
    if (so.split_n > 0) {
        const int old_cnt = r.cnt;
        split_reg(r, r2, so.split_n, qlen, so.split_rec >= 0 ? splits + so.split_rec : nullptr);
        has_r2 = r2.cnt > 0 && r.cnt != old_cnt;
        if (so.split_inv) r2.split_inv = 1;
    }
    r.rs = so.rs1; r.re = so.re1;
    if (r.rev) { r.qs = qlen - so.qe1; r.qe = qlen - so.qs1; }
    else { r.qs = so.qs1; r.qe = so.qe1; }
    // the CIGAR fix-up and the alignment statistics (mm_update_extra) are done for the whole round by aln_finish_wave_kernel
    r.fin_idx = r.has_p ? fin_idx : -1;
    r.aligned = 1;
    return has_r2;
}

void merge_regs(const mpn_map_opt *opt, int k, std::vector<Reg> &regs, int32_t rep_len) {
    if (regs.empty()) return;
    for (Reg &r : regs) { r.subsc = 0; r.n_sub = 0; if (r.has_p) r.dp_max2 = 0; }
    hit_sort(regs);
    set_parent(opt->mask_level, regs, opt->a * 2 + opt->b);
    select_sub(opt->pri_ratio, k * 2, opt->best_n, regs);
    set_sam_pri(regs);
    set_mapq(regs, opt->min_chain_score, opt->a, rep_len);
}

}  // namespace mpn
