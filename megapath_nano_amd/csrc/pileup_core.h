// The arithmetic behind include/mpn_pileup.h that is the same on the device and on the host: what a record's CIGAR says
// (pile_record), the counts of one record taken serially (pile_count_serial: the host check and the statement of what the wave
// of pile_counts_kernel computes), and the decision on one position (pile_decide).  Written from Clair's
// preprocess/ExtractVariantCandidates.py as DESIGN.md section 6 restates it.  It compiles for the device (csrc/pileup_kernels.hip)
// and for the host (scripts/pileup_host_check.cpp runs the golden cases and malformed records through it under the sanitizers).
//
// Bounds: every read is of text[a .. a + k) with a + k <= len checked in 64-bit arithmetic before it; a base is read only at a
// query index below l_seq, and the packed bases are known to lie inside the text before the first of them is read.
#pragma once
#include <stdint.h>
#include "../../include/mpn_pileup.h"
#include "bam_walk_core.h"

#if defined(__HIPCC__)
#define PILE_HD __host__ __device__ inline
#else
#define PILE_HD inline
#endif

namespace mpn_pile {

using mpn_bamw::bamw_i32;
using mpn_bamw::bamw_u16;
using mpn_bamw::BAMW_FIXED;

enum { PILE_A = 0, PILE_C = 1, PILE_G = 2, PILE_T = 3, PILE_I = 4, PILE_D = 5, PILE_N = 6, PILE_NONE = 15 };
enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5, OP_P = 6, OP_EQ = 7, OP_X = 8 };

// the slot of a 4-bit base code (=ACMGRSVTWYHKDBN), four bits each, code 0 first: '=' has none
constexpr uint64_t PILE_SLOT_OF_CODE = 0x610201030102010Full;
PILE_HD int pile_slot(uint32_t code) { return (int)((PILE_SLOT_OF_CODE >> (4 * (code & 15u))) & 15u); }

PILE_HD bool pile_is_match(uint32_t op) { return op == OP_M || op == OP_EQ || op == OP_X; }
PILE_HD uint32_t pile_u32(const uint8_t *t, int64_t a) { return (uint32_t)bamw_i32(t, a); }

// The reference byte as the script reads it: one of the upper-case letters ACGTURYSWKMBDHVN mapped to A, C, G, T or N; 0 for any
// other byte (lower case included): the position is skipped.
PILE_HD uint8_t pile_ref_base(uint8_t b) {
    switch (b) {
        case 'A': case 'R': case 'W': case 'M': case 'D': case 'H': case 'V': return 'A';
        case 'C': case 'Y': case 'S': case 'B': return 'C';
        case 'G': case 'K': return 'G';
        case 'T': case 'U': return 'T';
        case 'N': return 'N';
        default: return 0;
    }
}

// Where the pieces of the record at text[off] lie; false if its fixed bytes, its CIGAR or its packed bases pass the end of the
// record or of the text.
struct PileLayout { int64_t cigar, seq; int32_t n_cigar, l_seq; };
PILE_HD bool pile_layout(const uint8_t *t, int64_t len, int64_t off, PileLayout *L) {
    if (off < 0 || off > len - BAMW_FIXED) return false;
    const int64_t end = off + 4 + (int64_t)bamw_i32(t, off);
    L->n_cigar = (int32_t)bamw_u16(t, off + 16);
    L->l_seq = bamw_i32(t, off + 20);
    L->cigar = off + BAMW_FIXED + (int64_t)t[off + 12];
    L->seq = L->cigar + 4 * (int64_t)L->n_cigar;
    if (L->l_seq < 0) return false;
    const int64_t seq_end = L->seq + ((int64_t)L->l_seq + 1) / 2;
    return seq_end <= end && seq_end <= len;
}

// What the record at text[off] says (include/mpn_pileup.h mpn_pileup_rec).  off + 36 <= len is the caller's.
PILE_HD void pile_record(const uint8_t *t, int64_t len, int64_t off, mpn_pileup_rec *r) {
    r->soft = r->total = r->span = 0;
    r->ref_id = bamw_i32(t, off + 4);
    r->pos = bamw_i32(t, off + 8);
    r->mapq = t[off + 13];
    r->n_cigar = (uint16_t)bamw_u16(t, off + 16);
    r->status = MPN_PILEUP_OK;
    r->reserved = 0;
    PileLayout L;
    if (!pile_layout(t, len, off, &L)) { r->status = MPN_PILEUP_CIGAR_PAST; return; }
    int64_t query = 0;
    bool no_base = false;
    uint32_t first_op = 0, first_len = 0;
    for (int32_t k = 0; k < L.n_cigar; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        if (k == 0) { first_op = op; first_len = n; }
        if (op > 8) { r->status = MPN_PILEUP_BAD_OP; return; }
        if (k == 1 && L.n_cigar == 2 && op == OP_N && first_op == OP_S && first_len == (uint32_t)L.l_seq) {
            r->status = MPN_PILEUP_PLACEHOLDER;
            return;
        }
        r->total += n;
        if (op == OP_S) r->soft += n;
        if (pile_is_match(op) || op == OP_D) r->span += n;
        if (pile_is_match(op) || op == OP_I || op == OP_S) {
            query += n;
            if (pile_is_match(op) && n > 0 && query > L.l_seq) no_base = true;
        }
    }
    if (no_base) r->status = MPN_PILEUP_NO_BASE;
}

// The counts of the record at text[off] inside [lo, hi), added to counts[(p - lo) * 7 + slot], on one thread.  Returns 0, or 1
// for a record that does not lie inside the text, has an operation code above 8, or has code 0 or no base under an M, = or X
// (what was added up to there stays).
PILE_HD int pile_count_serial(const uint8_t *t, int64_t len, int64_t off, int32_t pos, int lead, int64_t lo, int64_t hi, int32_t *counts) {
    PileLayout L;
    if (!pile_layout(t, len, off, &L)) return 1;
    int64_t rp = pos, qp = 0;
    for (int32_t k = 0; k < L.n_cigar; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        if (op > 8) return 1;
        if (pile_is_match(op)) {
            for (uint32_t j = 0; j < n; ++j, ++rp, ++qp) {
                if (qp >= L.l_seq) return 1;
                const uint32_t byte = t[L.seq + (qp >> 1)];
                const int slot = pile_slot((qp & 1) ? byte : byte >> 4);
                if (slot == PILE_NONE) return 1;
                if (rp >= lo && rp < hi) ++counts[(rp - lo) * MPN_PILEUP_SLOTS + slot];
            }
        } else if (op == OP_I || op == OP_D) {
            const int64_t p = rp - 1;
            if ((rp != pos || lead) && p >= lo && p < hi) ++counts[(p - lo) * MPN_PILEUP_SLOTS + (op == OP_I ? PILE_I : PILE_D)];
            if (op == OP_I) qp += n; else rp += n;
        } else if (op == OP_S) {
            qp += n;
        }
    }
    return 0;
}

// The decision on one position: c = its seven counters, ref_byte = the reference byte.  True: the position is a candidate and
// *out is its row (pos is the caller's).  Float64 division and compares, as the script does them.
PILE_HD bool pile_decide(const int32_t *c, uint8_t ref_byte, double min_coverage, double threshold, mpn_pileup_cand *out) {
    const uint8_t rb = pile_ref_base(ref_byte);
    if (!rb) return false;
    const int32_t depth = c[PILE_A] + c[PILE_C] + c[PILE_G] + c[PILE_T] + c[PILE_N];
    if ((double)depth < min_coverage) return false;
    const char letters[MPN_PILEUP_SLOTS + 1] = "ACGTIDN";
    int32_t cnt[MPN_PILEUP_SLOTS];
    uint8_t lab[MPN_PILEUP_SLOTS];
    for (int k = 0; k < MPN_PILEUP_SLOTS; ++k) {        // a stable insertion sort by descending count
        int j = k;
        for (; j > 0 && cnt[j - 1] < c[k]; --j) { cnt[j] = cnt[j - 1]; lab[j] = lab[j - 1]; }
        cnt[j] = c[k];
        lab[j] = (uint8_t)letters[k];
    }
    const double denominator = depth > 0 ? (double)depth : 1.0;
    if (!(lab[0] != rb || (double)cnt[1] / denominator >= threshold)) return false;
    out->depth = depth;
    out->ref_base = rb;
    for (int k = 0; k < MPN_PILEUP_SLOTS; ++k) { out->count[k] = cnt[k]; out->label[k] = lab[k]; }
    return true;
}

}  // namespace mpn_pile
