// The arithmetic behind include/mpn_read_realign.h that is the same on the device and on the host, written from
// realignment/realign_illumina_reads.py as DESIGN.md section 6 restates it: what a record says (rr_record, the aux walk
// included), the chunk recurrence (rr_chunks_serial), the rules of the pileup[...]["X"] counter (rr_base_counts, rr_in_region,
// rr_before_ok) with the counts of one record taken serially (rr_support_serial: the host check and the statement of what a wave
// of rr_support_kernel computes), and find_max_overlap_index (rr_assign_one).  It compiles for the device
// (csrc/read_realign_kernels.hip) and for the host (scripts/read_realign_host_check.cpp, under the sanitizers).
//
// The rules of the counter, for a record with MAPQ >= 20 (RR_MIN_MQ) only:
//   =        moves both positions and counts nothing
//   M, X     per base: one at its position if the raw quality is >= 20, the contig's byte is one of ACGT and differs from the
//            read's letter (the letter of the 4-bit code, =ACMGRSVTWYHKDBN)
//   I, S     at reference position p with length n: one at every position of [p - n, p + n) if p lies inside
//            [chunk_start - 20, chunk_start + 5020] of the chunk that is current when the record is parsed, the contig's byte
//            before p is one of ACGT (at p = 0 that is the contig's LAST byte: Python's index -1) and all n qualities are >= 20
//   D        one at every position of [p, p + n) under the first two of these, then the reference position moves on
//   N, H, P  nothing at all: N does NOT move the reference position
// Positions may be negative (a leading clip at POS < its length): a row is indexed from its own first position.
//
// Bounds: as in pileup_core.h; a base or quality is read only at a query index below l_seq, bases and qualities are known to lie
// inside the text before the first is read, an aux field only inside its record, and a contig byte only at an index inside
// [0, contig_len).
#pragma once
#include <stdint.h>
#include "../../include/mpn_read_realign.h"
#include "tensor_core.h"

#define RR_HD PILE_HD

namespace mpn_rr {

using namespace mpn_tens;

constexpr int RR_ROW = MPN_RR_ROW, RR_CHUNK = MPN_RR_CHUNK, RR_EXPAND = MPN_RR_EXPAND;
static_assert(RR_ROW == RR_CHUNK + 2 * RR_EXPAND + 1, "chunk_start - 21 .. chunk_end + 19");

RR_HD bool rr_acgt(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }
// the letter samtools prints for a 4-bit base code
RR_HD uint8_t rr_letter(uint32_t code) {
    const char letters[17] = "=ACMGRSVTWYHKDBN";
    return (uint8_t)letters[code & 15u];
}

// ---- records -------------------------------------------------------------------------------------------------------------------
// The aux fields text[a .. end) of one record.  *hp: see mpn_rr_rec.  Returns MPN_RR_OK, _PAST, _BAD_AUX or _HP_TEXT: the first
// that the walk meets.
RR_HD int rr_aux(const uint8_t *t, int64_t a, int64_t end, uint8_t *hp) {
    bool found = false;
    *hp = 0;
    while (a < end) {
        if (a + 3 > end) return MPN_RR_PAST;
        const uint8_t t0 = t[a], t1 = t[a + 1], ty = t[a + 2];
        a += 3;
        int64_t size = 0;
        bool integer = false;
        switch (ty) {
            case 'c': case 'C': integer = true; size = 1; break;
            case 'A': size = 1; break;
            case 's': case 'S': integer = true; size = 2; break;
            case 'i': case 'I': integer = true; size = 4; break;
            case 'f': size = 4; break;
            case 'Z': case 'H': {
                int64_t z = a;
                int run = 0;                    // how much of `HP:i:` the bytes before z spell
                bool hit = false;
                while (z < end && t[z]) {
                    const uint8_t c = t[z];
                    const char want[6] = "HP:i:";
                    run = c == (uint8_t)want[run] ? run + 1 : (c == 'H' ? 1 : 0);
                    if (run == 5) { hit = true; run = 0; }
                    ++z;
                }
                if (z >= end) return MPN_RR_PAST;
                if (hit) return MPN_RR_HP_TEXT;
                a = z + 1;
                continue;
            }
            case 'B': {
                if (a + 5 > end) return MPN_RR_PAST;
                const uint8_t sub = t[a];
                const int64_t count = (int64_t)pile_u32(t, a + 1);
                int64_t es = 0;
                switch (sub) {
                    case 'c': case 'C': es = 1; break;
                    case 's': case 'S': es = 2; break;
                    case 'i': case 'I': case 'f': es = 4; break;
                    default: return MPN_RR_BAD_AUX;
                }
                if (count * es > end - a - 5) return MPN_RR_PAST;
                a += 5 + count * es;
                continue;
            }
            default: return MPN_RR_BAD_AUX;
        }
        if (a + size > end) return MPN_RR_PAST;
        if (integer && !found && t0 == 'H' && t1 == 'P') {
            found = true;
            int64_t v = 0;
            switch (ty) {
                case 'c': v = (int8_t)t[a]; break;
                case 'C': v = t[a]; break;
                case 's': v = (int16_t)bamw_u16(t, a); break;
                case 'S': v = bamw_u16(t, a); break;
                case 'i': v = bamw_i32(t, a); break;
                default: v = (int64_t)pile_u32(t, a); break;
            }
            if (v >= 0) {
                while (v >= 10) v /= 10;
                *hp = (uint8_t)('0' + v);
            }
        }
        a += size;
    }
    return MPN_RR_OK;
}

// is_too_many_soft_clipped_bases_for_a_read_from, in float64 as the script writes it: the one statement of the rule, which
// rr_record leaves in mpn_rr_rec.clipped for the host check and the Python layer alike
RR_HD bool rr_too_clipped(int64_t soft, int64_t total) { return 1.0 - (double)soft / (double)(total + 1) < 0.55; }

// What the record at text[off] says (mpn_rr_rec).  off + 36 <= len is the caller's.
RR_HD void rr_record(const uint8_t *t, int64_t len, int64_t off, mpn_rr_rec *r) {
    r->soft = r->total = r->del = r->span = 0;
    r->ref_id = bamw_i32(t, off + 4);
    r->pos = bamw_i32(t, off + 8);
    r->mapq = t[off + 13];
    r->n_cigar = (uint16_t)bamw_u16(t, off + 16);
    r->flag = (uint16_t)bamw_u16(t, off + 18);
    r->l_seq = bamw_i32(t, off + 20);
    r->next_ref = bamw_i32(t, off + 24);
    r->next_pos = bamw_i32(t, off + 28);
    r->has_seq = r->has_qual = r->hp = r->clipped = 0;
    r->status = MPN_RR_OK;
    r->reserved[0] = r->reserved[1] = 0;
    TensLayout L;
    const int64_t end = off + 4 + (int64_t)bamw_i32(t, off);
    if (!tens_layout(t, len, off, &L) || end > len) { r->status = MPN_RR_PAST; return; }
    r->has_seq = L.l_seq > 0;
    r->has_qual = L.l_seq > 0 && t[L.qual] != 0xff;
    int64_t query = 0;
    uint32_t first_op = 0, first_len = 0;
    for (int32_t k = 0; k < L.n_cigar; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        if (k == 0) { first_op = op; first_len = n; }
        if (op > 8) { r->status = MPN_RR_BAD_OP; return; }
        if (k == 1 && L.n_cigar == 2 && op == OP_N && first_op == OP_S && first_len == (uint32_t)L.l_seq) { r->status = MPN_RR_PLACEHOLDER; return; }
        r->total += n;
        if (op == OP_S) r->soft += n;
        if (op == OP_D) r->del += n;
        if (pile_is_match(op) || op == OP_D) r->span += n;
        if (pile_is_match(op) || op == OP_I || op == OP_S) query += n;
    }
    r->clipped = rr_too_clipped(r->soft, r->total);
    if (query > L.l_seq) { r->status = MPN_RR_NO_BASE; return; }
    for (int64_t q = 0; q < L.l_seq; ++q)
        if (tens_base_code(t, L, q) == 0) { r->status = MPN_RR_BASE_EQ; return; }
    r->status = (uint8_t)rr_aux(t, L.qual + (int64_t)L.l_seq, end, &r->hp);
}

// ---- the chunk recurrence -------------------------------------------------------------------------------------------------------
// mpn_rr_chunks.  chunk_end + 20 of chunk c is first + 5000 * (c + 1) + 20.
RR_HD void rr_chunks_serial(int64_t n, const int32_t *pos, int64_t *first, int64_t *chunk, int32_t *chunk_of) {
    for (int64_t i = 0; i < n; ++i) {
        if (*first < 0) *first = pos[i];
        if ((int64_t)pos[i] >= *first + (int64_t)RR_CHUNK * (*chunk + 1) + RR_EXPAND) ++*chunk;      // one yield, one step
        chunk_of[i] = (int32_t)*chunk;
    }
}

// ---- the counter ----------------------------------------------------------------------------------------------------------------
// an I, S or D at reference position p is inside the region of the chunk that starts at cs
RR_HD bool rr_in_region(int64_t p, int64_t cs) { return !(p < cs - RR_EXPAND || p > cs + RR_CHUNK + RR_EXPAND); }

// The base before p is one of ACGT.  -1: there is no such byte (p behind the contig's end, or an empty contig).
RR_HD int rr_before_ok(const uint8_t *contig, int64_t contig_len, int64_t p) {
    if (contig_len <= 0 || p < 0 || p > contig_len) return -1;
    return rr_acgt(contig[p == 0 ? contig_len - 1 : p - 1]) ? 1 : 0;
}

// One base of an M or X: query index q over position p.  1: it counts, 0: it does not, -1: the base or the contig byte is not there.
RR_HD int rr_base_counts(const uint8_t *t, const TensLayout &L, int64_t q, const uint8_t *contig, int64_t contig_len, int64_t p) {
    if (q < 0 || q >= L.l_seq || p < 0 || p >= contig_len) return -1;
    if (t[L.qual + q] < MPN_RR_MIN_BQ) return 0;
    const uint8_t rb = contig[p];
    return rr_acgt(rb) && rr_letter(tens_base_code(t, L, q)) != rb ? 1 : 0;
}

// The counts of the record at text[off] inside the row [lo, lo + RR_ROW), added to row[p - lo], on one thread.  Only what can
// reach the row is looked at.  Returns 0, or 1 for a record that does not lie inside the text, has an operation code above 8 or
// needs a base, a quality or a contig byte that is not there (what was added up to there stays).
RR_HD int rr_support_serial(const uint8_t *t, int64_t len, int64_t off, int32_t pos, int64_t chunk_start, const uint8_t *contig, int64_t contig_len,
                            int64_t lo, int32_t *row) {
    TensLayout L;
    if (!tens_layout(t, len, off, &L)) return 1;
    if (t[off + 13] < MPN_RR_MIN_MQ) return 0;
    const int64_t hi = lo + RR_ROW;
    int64_t rp = pos, qp = 0;
    for (int32_t k = 0; k < L.n_cigar; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u;
        const int64_t n = w >> 4;
        if (op > 8) return 1;
        if (op == OP_EQ) {
            rp += n; qp += n;
        } else if (op == OP_M || op == OP_X) {
            const int64_t s = rp > lo ? rp : lo, e = rp + n < hi ? rp + n : hi;
            for (int64_t p = s; p < e; ++p) {
                const int c = rr_base_counts(t, L, qp + (p - rp), contig, contig_len, p);
                if (c < 0) return 1;
                row[p - lo] += c;
            }
            rp += n; qp += n;
        } else if (op == OP_I || op == OP_S || op == OP_D) {
            const bool ins = op != OP_D;
            const int64_t a = ins ? rp - n : rp, b = rp + n;
            const int64_t s = a > lo ? a : lo, e = b < hi ? b : hi;
            if (n > 0 && e > s && rr_in_region(rp, chunk_start)) {
                const int before = rr_before_ok(contig, contig_len, rp);
                if (before < 0) return 1;
                bool good = before == 1;
                if (good && ins) {
                    if (qp + n > L.l_seq) return 1;
                    for (int64_t j = 0; j < n && good; ++j) good = t[L.qual + qp + j] >= MPN_RR_MIN_BQ;
                }
                if (good)
                    for (int64_t p = s; p < e; ++p) ++row[p - lo];
            }
            if (ins) qp += n; else rp += n;
        }
    }
    return 0;
}

// ---- find_max_overlap_index -----------------------------------------------------------------------------------------------------
// The window (0 .. n_win) of the sorted, disjoint windows [ws[w], we[w]) that the read [pos, end) goes to, or -1.
RR_HD int32_t rr_assign_one(int64_t pos, int64_t end, int32_t n_win, const int32_t *ws, const int32_t *we) {
    if (n_win <= 0) return -1;
    int64_t max_end = we[0];
    for (int32_t w = 1; w < n_win; ++w) max_end = we[w] > max_end ? we[w] : max_end;
    if (pos > max_end) return -1;
    int64_t best = 0;
    int32_t at = -1;
    for (int32_t w = 0; w < n_win; ++w) {
        const int64_t a = pos > ws[w] ? pos : ws[w], b = end < we[w] ? end : we[w];
        if (b - a > best) { best = b - a; at = w; }
    }
    return at;
}

}  // namespace mpn_rr
