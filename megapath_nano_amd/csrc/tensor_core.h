// The arithmetic behind include/mpn_tensor.h that is the same on the device and on the host: what a record says beyond
// pile_record (tens_record), whether a record joins a centre (tens_joins), what one CIGAR operation adds to a centre's tensor
// (tens_op) and whether it makes the read a high-quality one at the centre (tens_flag_op), and the serial walks over a record
// that state what a wave of the kernels computes (tens_fill_serial, tens_flag_serial).  Written from Clair's
// preprocess/CreateTensor.py as DESIGN.md section 6 restates it.  It compiles for the device (csrc/tensor_kernels.hip) and for the
// host (scripts/tensor_host_check.cpp runs the golden cases and malformed records through it under the sanitizers).
//
// The script keeps, per read and centre, the entries from the position at which the read joins the centre: join = max(POS, c0 - 16)
// with left edges, c0 - 16 without.  An M, = or X base is kept from `join` on; a D base only behind it (the script appends a D
// before it looks the position up); an I only when the next reference position lies behind it.
//
// Bounds: as in pileup_core.h; a base or quality is read only at a query index below l_seq, bases and qualities are known to lie
// inside the text before the first is read, and a reference byte is read only at an index inside [0, ref_len).
#pragma once
#include <stdint.h>
#include "../../include/mpn_tensor.h"
#include "pileup_core.h"

#define TENS_HD PILE_HD

namespace mpn_tens {

using namespace mpn_pile;

constexpr int FLANK = MPN_TENSOR_FLANK, NPOS = MPN_TENSOR_POSITIONS, ROWS = MPN_TENSOR_ROWS, CHANNELS = MPN_TENSOR_CHANNELS, CELLS = MPN_TENSOR_CELLS;
static_assert(NPOS * ROWS * CHANNELS == CELLS && NPOS == 2 * FLANK + 1, "the tensor");

// BASE2NUM (shared/utils.py IUPAC_base_to_num_dict) of a reference byte; -1: not one of the sixteen upper-case letters
TENS_HD int tens_ref_num(uint8_t b) {
    switch (b) {
        case 'A': case 'R': case 'W': case 'M': case 'D': case 'H': case 'V': case 'N': return 0;
        case 'C': case 'Y': case 'S': case 'B': return 1;
        case 'G': case 'K': return 2;
        case 'T': case 'U': return 3;
        default: return -1;
    }
}
// the same of a 4-bit base code (=ACMGRSVTWYHKDBN), four bits each, code 0 first: '=' has none (15)
constexpr uint64_t TENS_NUM_OF_CODE = 0x010201030102010Full;
TENS_HD int tens_code_num(uint32_t code) { return (int)((TENS_NUM_OF_CODE >> (4 * (code & 15u))) & 15u); }

// pile_layout and the qualities behind the bases
struct TensLayout { int64_t cigar, seq, qual; int32_t n_cigar, l_seq; };
TENS_HD bool tens_layout(const uint8_t *t, int64_t len, int64_t off, TensLayout *L) {
    PileLayout P;
    if (!pile_layout(t, len, off, &P)) return false;
    L->cigar = P.cigar; L->seq = P.seq; L->n_cigar = P.n_cigar; L->l_seq = P.l_seq;
    L->qual = P.seq + ((int64_t)P.l_seq + 1) / 2;
    const int64_t end = off + 4 + (int64_t)bamw_i32(t, off), qual_end = L->qual + (int64_t)P.l_seq;
    return qual_end <= end && qual_end <= len;
}

// What the record at text[off] says (mpn_tensor_rec).  off + 36 <= len is the caller's.
TENS_HD void tens_record(const uint8_t *t, int64_t len, int64_t off, mpn_tensor_rec *r) {
    r->hts_len = 0; r->l_seq = 0; r->has_qual = 0; r->status = MPN_PILEUP_OK; r->reserved = 0;
    TensLayout L;
    if (!tens_layout(t, len, off, &L)) { r->status = MPN_PILEUP_CIGAR_PAST; return; }
    r->l_seq = L.l_seq;
    r->has_qual = L.l_seq > 0 && t[L.qual] != 0xff;
    int64_t query = 0;
    bool no_base = false;
    for (int32_t k = 0; k < L.n_cigar; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        if (op > 8) { r->status = MPN_PILEUP_BAD_OP; return; }
        if (pile_is_match(op) || op == OP_D || op == OP_N) r->hts_len += n;
        if (pile_is_match(op) || op == OP_I || op == OP_S) {
            query += n;
            if (pile_is_match(op) && n > 0 && query > L.l_seq) no_base = true;
        }
    }
    if (no_base) r->status = MPN_PILEUP_NO_BASE;
}

TENS_HD bool tens_joins(int64_t pos, int64_t span, int64_t c0, int left_edge) {
    if (span <= 0) return false;
    const int64_t a = c0 - FLANK;
    return left_edge ? (pos <= c0 + FLANK + 1 && pos + span > a) : (pos <= a && pos + span > a);
}
TENS_HD int64_t tens_join_pos(int64_t pos, int64_t c0, int left_edge) { return left_edge && pos > c0 - FLANK ? pos : c0 - FLANK; }

// A centre, where the read joined it, and the reference bytes.
struct TensWin { int64_t c0, join; const uint8_t *ref; int64_t ref_start, ref_len; };

TENS_HD uint32_t tens_base_code(const uint8_t *t, const TensLayout &L, int64_t q) {
    const uint32_t byte = t[L.seq + (q >> 1)];
    return ((q & 1) ? byte : byte >> 4) & 15u;
}

// What one operation (op, length n, starting at reference position r0 and query index q0) of a read adds: add(cell) once per
// count.  Returns 0, or 1 if a base that counts does not exist or a reference byte of the window does not.
template <class Add>
TENS_HD int tens_op(const uint8_t *t, const TensLayout &L, uint32_t op, int64_t n, int64_t r0, int64_t q0, int strand, const TensWin &W, Add &add) {
    const int64_t last = W.c0 + FLANK;                 // the last position with a tensor index
    if (pile_is_match(op) || op == OP_D) {
        const bool match = pile_is_match(op);
        const int64_t from = match ? W.join : W.join + 1;
        const int64_t s = r0 > from ? r0 : from, e = r0 + n < last + 1 ? r0 + n : last + 1;
        for (int64_t p = s; p < e; ++p) {
            const int64_t ri = p - W.ref_start;
            if (ri < 0 || ri >= W.ref_len) return 1;
            const int rn = tens_ref_num(W.ref[ri]);
            const int cell = (int)(p - W.c0 + FLANK) * ROWS * CHANNELS;
            if (!match) {
                if (rn >= 0) add(cell + (rn + strand) * CHANNELS + 2);
                continue;
            }
            const int64_t q = q0 + (p - r0);
            if (q >= L.l_seq) return 1;
            const int qn = tens_code_num(tens_base_code(t, L, q));
            if (rn < 0 || qn == 15) continue;
            add(cell + (rn + strand) * CHANNELS + 0);
            add(cell + (qn + strand) * CHANNELS + 1);
            add(cell + (rn + strand) * CHANNELS + 2);
            add(cell + (qn + strand) * CHANNELS + 3);
        }
    } else if (op == OP_I && r0 > W.join && r0 <= last) {
        const int64_t index = r0 - W.c0 + FLANK;
        for (int64_t k = 0; k < n; ++k) {
            if (q0 + k >= L.l_seq) return 1;
            const int qn = tens_code_num(tens_base_code(t, L, q0 + k));
            if (qn == 15) continue;
            const int64_t at = index + k < NPOS - 1 ? index + k : NPOS - 1;
            add((int)at * ROWS * CHANNELS + (qn + strand) * CHANNELS + 1);
        }
    }
    return 0;
}

// 1: the operation gives the read a high-quality base at the centre; 0: it does not; -1: the base does not exist
TENS_HD int tens_flag_op(const uint8_t *t, const TensLayout &L, uint32_t op, int64_t n, int64_t r0, int64_t q0, const TensWin &W) {
    if (!(r0 <= W.c0 && W.c0 < r0 + n)) return 0;
    if (op == OP_D) return W.c0 > W.join ? 1 : 0;
    if (!pile_is_match(op) || W.c0 < W.join) return 0;
    const int64_t q = q0 + (W.c0 - r0);
    if (q >= L.l_seq) return -1;
    return t[L.qual + q] >= MPN_TENSOR_QUAL ? 1 : 0;
}

struct TensPlainAdd {
    int32_t *tile;
    TENS_HD void operator()(int cell) { ++tile[cell]; }
};

// The counts of the record at text[off] for the centre c0, added to tile[CELLS], on one thread.  Returns 0, or 1 for a record that
// does not lie inside the text, has an operation code above 8, or lacks a base or a reference byte that counts.
TENS_HD int tens_fill_serial(const uint8_t *t, int64_t len, int64_t off, int64_t pos, int reverse, int64_t c0, int left_edge, const uint8_t *ref,
                             int64_t ref_start, int64_t ref_len, int32_t *tile) {
    TensLayout L;
    if (!tens_layout(t, len, off, &L)) return 1;
    const TensWin W{c0, tens_join_pos(pos, c0, left_edge), ref, ref_start, ref_len};
    TensPlainAdd add{tile};
    int64_t rp = pos, qp = 0;
    for (int32_t k = 0; k < L.n_cigar && rp <= c0 + FLANK; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        if (op > 8) return 1;
        if (tens_op(t, L, op, (int64_t)n, rp, qp, reverse ? 4 : 0, W, add)) return 1;
        if (pile_is_match(op) || op == OP_D) rp += n;
        if (pile_is_match(op) || op == OP_I || op == OP_S) qp += n;
    }
    return 0;
}

// 1 / 0: the flag of mpn_tensor_centre_flags; -1: a record as above
TENS_HD int tens_flag_serial(const uint8_t *t, int64_t len, int64_t off, int64_t pos, int64_t c0, int left_edge) {
    TensLayout L;
    if (!tens_layout(t, len, off, &L)) return -1;
    const TensWin W{c0, tens_join_pos(pos, c0, left_edge), nullptr, 0, 0};
    int64_t rp = pos, qp = 0;
    for (int32_t k = 0; k < L.n_cigar && rp <= c0; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        if (op > 8) return -1;
        const int f = tens_flag_op(t, L, op, (int64_t)n, rp, qp, W);
        if (f) return f;
        if (pile_is_match(op) || op == OP_D) rp += n;
        if (pile_is_match(op) || op == OP_I || op == OP_S) qp += n;
    }
    return 0;
}

// decimal digits of a value that is not negative
TENS_HD int tens_digits(uint32_t v) {
    int d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}
// writes v in decimal at out[at ..) where at + digits <= cap; returns the digits
TENS_HD int tens_put(uint8_t *out, int64_t at, int64_t cap, uint32_t v) {
    const int d = tens_digits(v);
    for (int k = d - 1; k >= 0; --k) {
        if (at + k < cap) out[at + k] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    return d;
}

}  // namespace mpn_tens
