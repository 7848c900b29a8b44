// The mapper's per-read hit bookkeeping on the host: minimap2's hit.c (mm_gen_regs, mm_set_parent, mm_select_sub, mm_squeeze_a,
// mm_join_long, mm_hit_sort, mm_set_mapq, mm_split_reg, the merge of a split index' parts) on the chain records the chain stage
// leaves, and the accumulator of a batch's hits over index parts with its wire format (hits_block.cpp).  Host only: no HIP
// include, so that a host compiler builds these units and scripts/hit_host_check.cpp runs them under the sanitizers.
#pragma once
#include "map_records.h"
#include "../../include/mpn_map.h"

#include <stdint.h>
#include <string>
#include <utility>
#include <vector>

namespace mpn {

void set_error(const char *fmt, ...);   // (mpn_runtime.hip; declared here again so that mpn_common.h, which needs HIP, stays out)

static const int PARENT_UNSET = -1, PARENT_TMP_PRI = -2;

struct Reg {
    int32_t id = 0, cnt = 0, rid = 0, score = 0, qs = 0, qe = 0, rs = 0, re = 0, parent = PARENT_UNSET, subsc = 0, as = 0;
    int32_t mlen = 0, blen = 0, n_sub = 0, score0 = 0;
    uint32_t mapq = 0, split = 0, rev = 0, inv = 0, sam_pri = 0, split_inv = 0, hash = 0;
    int32_t has_p = 0, dp_score = 0, dp_max = 0, dp_max2 = 0, n_ambi = 0;
    std::vector<uint32_t> cigar;   // with MPN_TAG_EQX: its M ops already split into = (7) and X (8)
    std::string cs, md;            // cs:Z / MD:Z strings of the alignment (tag_kernels.h), when the call asked for them
    int32_t aligned = 0;  // base-level extension already done (or not needed)
    int32_t fin_qs = 0, fin_rs = 0, fin_ql = 0, fin_tl = 0;   // an inversion hit before its extension: the window to extend
    int32_t fin_idx = -1;  // >= 0: stitched this round (its index among the round's hits): CIGAR fix-up and statistics are due
    // The hit's first and last chained anchor (the anchors themselves stay in HBM: chain_backtrack_kernel's ChainRec) and, until
    // the squeeze, where its chain lies in the chain stage's pool (relative to the read's b_pos) and its segment of the squeeze
    uint64_t fx = 0, fy = 0, lx = 0, ly = 0;
    int64_t src = 0;
    int32_t seg = -1;
};

struct ReadState {
    std::vector<Reg> regs;
    int n_a = 0;           // anchors of the read's squeezed list (which lives in HBM)
    std::vector<int> pending; // reg indices aligned this round
};

// mm_reg_set_coor from the hit's first and last anchor (the approximate lengths of mm_cal_fuzzy_len come with the chain
// record, or are combined from two hits' when they are joined)
inline void reg_set_coor(Reg &r, int32_t qlen) {
    r.rev = (uint32_t)coor_rev(r.fx);
    r.rid = coor_rid(r.fx);
    r.rs = coor_rs(r.fx, r.fy);
    r.re = coor_re(r.lx);
    r.qs = coor_qs(r.fx, r.fy, r.ly, qlen);
    r.qe = coor_qe(r.fx, r.fy, r.ly, qlen);
}

inline void set_sam_pri(std::vector<Reg> &r) {
    int n_pri = 0;
    for (auto &x : r)
        if (x.id == x.parent) { ++n_pri; x.sam_pri = (n_pri == 1); }
        else x.sam_pri = 0;
}

// Per-thread scratch of the per-read hit bookkeeping: a few hundred thousand reads per step each need a handful of small
// arrays; allocating them per read costs more than the work on them.
struct HitScratch {
    std::vector<uint64_t> cov;
    std::vector<int> w, idx;
    std::vector<std::pair<uint64_t, int>> aux;
    std::vector<int32_t> order;
    std::vector<int64_t> src;
};
extern thread_local HitScratch tl_hs;

// Chain c of a read in the order of the first anchors (the order minimap2's chaining leaves them in, HostChains::chain_order):
// its (score, count) word, its record and the start of its anchors relative to the read's slice of the chain pool
struct ChainIn { uint64_t u; const ChainRec *rec; int64_t src; };

void gen_regs(uint32_t hash, int qlen, int n_u, const ChainIn *c, std::vector<Reg> &regs);
void set_parent(float mask_level, std::vector<Reg> &r, int sub_diff);
void select_sub(float pri_ratio, int min_diff, int best_n, std::vector<Reg> &r);
void filter_regs(const mpn_map_opt *opt, int qlen, std::vector<Reg> &regs);
// mm_squeeze_a: the hits that survived selection get consecutive places in the read's anchor list, in the order of their first
// anchors.  The anchors themselves are moved on the device (anchor_squeeze_kernel) along the segments written here: every hit
// is still ONE chain at this point.  Returns the anchors the list holds.
// (the read's segments are appended to `segs`, the staging list of the calling pool thread; Reg::seg indexes it)
int squeeze_a(std::vector<Reg> &regs, int read, int64_t pool_base, std::vector<SqueezeSeg> &segs);
// (called on a squeezed list: squeeze_a above has run)
void join_long(const mpn_map_opt *opt, int qlen, std::vector<Reg> &regs, std::vector<SqueezeSeg> &segs);
void hit_sort(std::vector<Reg> &r);
void set_mapq(std::vector<Reg> &regs, int min_chain_sc, int match_sc, int rep_len);
// What the stitching kernel found for one hit (stitch_kernels.h) applied to the hit: coordinates, DP score, and -- when a
// gap fill z-dropped -- the split of the hit at the last anchor before the drop (mm_align1's `dropped` branch; the kernel
// has located the anchor).  returns true if a split remainder was produced in r2
bool apply_stitch(int qlen, Reg &r, Reg &r2, const SplitRec *splits, const StitchOut &so, int fin_idx);
// minimap2's merge of the per-part hits of a read (mm_split_merge): the sub-optimal bookkeeping is reset, the hits are
// ranked, grouped and trimmed again over all parts, and MAPQ is recomputed
void merge_regs(const mpn_map_opt *opt, int k, std::vector<Reg> &regs, int32_t rep_len);

}  // namespace mpn

// Hits of a batch accumulated over the parts of a split index (minimap2 -I / --split-prefix): per read the hits of every
// part with target ids shifted to the concatenated target table, and the largest repetitive-seed span.
struct mpn_hits {
    int32_t n_reads = 0, n_parts = 0, k = 15;
    int32_t want_text = 1;   // 0: mpn_hits_finish will be asked for columns only: the CIGARs need not leave the GPU (mpn_hits_set_text)
    std::vector<std::vector<mpn::Reg>> regs;
    std::vector<int32_t> rep_len;
    std::vector<std::string> names;
    std::vector<int32_t> lens;
    int32_t tags = 0;        // MPN_TAG_* outputs the accumulated hits carry (made while each part was resident)
};
