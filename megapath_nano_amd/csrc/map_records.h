// Plain records and small pure functions of the mapper that the kernels and the host-only units (hit_host.cpp, aln_text.cpp,
// hits_block.cpp) share.  No HIP include: a host compiler takes this header as it is.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MPN_HD __host__ __device__
#else
#define MPN_HD
#endif

namespace mpn {

struct u128 { uint64_t x, y; };

// What the host needs of a chain to make a hit of it (minimap2's mm_reg1_t before the base-level extension): its first and
// last anchor and the approximate match / block lengths (mm_reg_set_coor + mm_cal_fuzzy_len).  The chained anchors themselves
// stay in HBM; chain_backtrack_kernel writes one record per surviving chain beside the (score, count) word.
struct ChainRec { uint64_t fx, fy, lx, ly; int32_t mlen, blen; };

// One surviving chain of a read on its way into the read's squeezed anchor list (minimap2's mm_squeeze_a after hit selection):
// cnt anchors from src (index into the chain stage's pool) to sq_off[read] + dst; flag: the first anchor gets SEED_LONG_JOIN.
struct SqueezeSeg { int64_t src; int32_t dst, cnt, read, flag; };

// The split of a z-dropped hit (mm_split_reg) as the host needs it: fuzzy lengths of both halves and the first anchor of the
// remainder.  Written by stitch_kernel for the hits it cuts.
struct SplitRec { uint64_t fx, fy, lx_left, ly_left; int32_t mlen_l, blen_l, mlen_r, blen_r; };

// What stitch_kernel leaves for one hit (stitch_kernels.h); apply_stitch (hit_host.h) applies it to the hit
struct StitchOut {
    int64_t cig_off;                  // start of the stitched CIGAR in the round's pool
    int32_t n_ops, dp_score, rs1, re1, qs1, qe1;
    int32_t has_p, dropped, drop_fill, drop_max_t, drop_max_q;   // drop_fill: index of the z-dropped gap fill among the hit's fills
    int32_t split_n;                  // > 0: a z-drop cuts the hit after its first split_n anchors (mm_align1's mm_split_reg call)
    int32_t split_inv, split_rec;     // the cut is at an inversion: the remainder is marked (mm_align1: r2->split_inv = 1); index of the hit's SplitRec
};

MPN_HD inline uint64_t hash64(uint64_t key) {
    key = ~key + (key << 21);
    key = key ^ key >> 24;
    key = (key + (key << 3)) + (key << 8);
    key = key ^ key >> 14;
    key = (key + (key << 2)) + (key << 4);
    key = key ^ key >> 28;
    key = key + (key << 31);
    return key;
}
MPN_HD inline uint32_t wang32(uint32_t key) {
    key += ~(key << 15); key ^= (key >> 10); key += (key << 3);
    key ^= (key >> 6); key += ~(key << 11); key ^= (key >> 16);
    return key;
}
MPN_HD inline uint32_t x31_hash(const char *s) {
    uint32_t h = (uint32_t)(unsigned char)*s;
    if (h) for (++s; *s; ++s) h = (h << 5) - h + (uint32_t)(unsigned char)*s;
    return h;
}

// mm_reg_set_coor: a hit's coordinates from the words of its first (fx, fy) and last (lx, ly) anchor and the read's length
MPN_HD inline int32_t coor_span(uint64_t fy) { return (int32_t)(fy >> 32 & 0xff); }
MPN_HD inline int32_t coor_rev(uint64_t fx) { return (int32_t)(fx >> 63); }
MPN_HD inline int32_t coor_rid(uint64_t fx) { return (int32_t)(fx << 1 >> 33); }
MPN_HD inline int32_t coor_rs(uint64_t fx, uint64_t fy) { return (int32_t)fx + 1 > coor_span(fy) ? (int32_t)fx + 1 - coor_span(fy) : 0; }
MPN_HD inline int32_t coor_re(uint64_t lx) { return (int32_t)lx + 1; }
MPN_HD inline int32_t coor_qs(uint64_t fx, uint64_t fy, uint64_t ly, int32_t qlen) {
    return !coor_rev(fx) ? (int32_t)fy + 1 - coor_span(fy) : qlen - ((int32_t)ly + 1);
}
MPN_HD inline int32_t coor_qe(uint64_t fx, uint64_t fy, uint64_t ly, int32_t qlen) {
    return !coor_rev(fx) ? (int32_t)ly + 1 : qlen - ((int32_t)fy + 1 - coor_span(fy));
}

}  // namespace mpn
