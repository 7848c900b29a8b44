// The arithmetic behind include/mpn_local_realign.h that is the same on the device and on the host: samtools' depth rule
// (lr_depth_rule, host), what one CIGAR operation says about a site's columns (lr_cover_op, lr_hazard_op, lr_finish_mask) and appends to a read's
// fragment (lr_frag_op), the allele keys of one read from its SSW result (lr_pair_keys), how two keys compare (lr_key_equal), and the
// serial walks that state what a wave of the kernels computes (lr_cover_serial, lr_frag_serial).  Written from the reference's
// realignment/local_realignment.py, pyssw.py and samtools mpileup's text as DESIGN.md section 6 item 20 restates them.  It compiles
// for the device (csrc/local_realign_kernels.hip) and for the host (scripts/local_realign_host_check.cpp runs the golden cases and
// malformed records through it under the sanitizers).
//
// Positions are 0-based here: a site at the 1-based position pos has the columns w0 .. w0 + 400 with w0 = pos - 201, and bit d of
// its mask is column w0 + d.
//
// Bounds: as in pileup_core.h and tensor_core.h; a base is read only at a query index below l_seq, a CIGAR word only at an index
// inside [0, n_cigar), a contig byte only at an index inside [0, contig_len).
#pragma once
#include <stdint.h>
#include "../../include/mpn_local_realign.h"
#include "tensor_core.h"

#define LR_HD TENS_HD

namespace mpn_lr {

using namespace mpn_tens;

constexpr int WINDOW = MPN_LR_WINDOW, REGION = MPN_LR_REGION, FLANK_REF = MPN_LR_FLANK, COLS = MPN_LR_COLUMNS, WORDS = MPN_LR_MASK_WORDS;
constexpr int MAX_KEYS = MPN_LR_MAX_KEYS;
static_assert(COLS == 2 * WINDOW + 1 && WORDS * 32 >= COLS, "the window");

LR_HD uint8_t lr_letter(uint32_t code) {
    const char letters[17] = "=ACMGRSVTWYHKDBN";
    return (uint8_t)letters[code & 15u];
}
LR_HD bool lr_acgt(uint32_t code) { return code == 1 || code == 2 || code == 4 || code == 8; }
LR_HD bool lr_known(uint32_t code) { return lr_acgt(code) || code == 15; }           // the letters decode_pileup_bases knows: ACGTN
LR_HD uint8_t lr_upper(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }
// pyssw's to_int of a letter (upper or lower case): A C G T -> 0 1 2 3, anything else is N
LR_HD int8_t lr_ssw_code(uint8_t b) {
    switch (lr_upper(b)) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return 4;
    }
}
LR_HD bool lr_bit(const uint32_t *mask, int64_t d) { return d >= 0 && d < COLS && ((mask[d >> 5] >> (d & 31)) & 1u); }
LR_HD int64_t lr_w0(int64_t pos1) { return pos1 - WINDOW - 1; }

// an N that overlaps the 0-based region [pos1 - 234, pos1 + 234), or a P that stands inside it
LR_HD bool lr_skip_or_pad(uint32_t op, int64_t n, int64_t r0, int64_t pos1) {
    const int64_t lo = pos1 - REGION - 1, hi = pos1 + REGION + 1;
    if (op == OP_N) return r0 < hi && r0 + n > lo;
    if (op == OP_P) return r0 >= lo && r0 <= hi;
    return false;
}

// What the operation (op, length n, from reference r0 and query q0) says about the columns of the window that starts at w0:
// orr(word, cov, bad) for every word of the mask it touches (cov: covered; bad: a matched base that is not one of ACGTN).
template <class Or>
LR_HD int lr_cover_op(const uint8_t *t, const TensLayout &L, uint32_t op, int64_t n, int64_t r0, int64_t q0, int64_t w0, Or &orr) {
    const bool match = pile_is_match(op);
    if (!match && op != OP_D) return MPN_LR_OK;
    const int64_t a = r0 > w0 ? r0 : w0, b = r0 + n < w0 + COLS ? r0 + n : w0 + COLS;
    uint32_t cov = 0, bad = 0;
    int word = -1;
    for (int64_t r = a; r < b; ++r) {
        const int d = (int)(r - w0);
        if ((d >> 5) != word) {
            if (word >= 0) orr(word, cov, bad);
            word = d >> 5; cov = bad = 0;
        }
        cov |= 1u << (d & 31);
        if (match) {
            const int64_t q = q0 + (r - r0);
            if (q >= L.l_seq) return MPN_LR_PAST_BASES;
            const uint32_t code = tens_base_code(t, L, q);
            if (code == 0) return MPN_LR_EQ_BASE;
            if (!lr_known(code)) bad |= 1u << (d & 31);
        }
    }
    if (word >= 0) orr(word, cov, bad);
    return MPN_LR_OK;
}

// The column at which the script's decode_pileup_bases may raise, or -1: a matched stretch that ends inside the site's region with a
// base that is not one of ACGTN, directly followed by an I or a D.  mpileup spells `w+1a` there; the parser has no entry for `w` and
// hangs the indel on the entry before it -- and raises IndexError if the row has none yet, that is if no earlier read of the pile-up
// gives an entry at the column (lr_entry_at).  Otherwise the row is merely dropped, as lr_cover_op has it.
LR_HD int64_t lr_hazard_op(const uint8_t *t, const TensLayout &L, int32_t k, uint32_t op, int64_t n, int64_t r0, int64_t q0, int64_t pos1) {
    if (!pile_is_match(op) || n <= 0 || k + 1 >= L.n_cigar) return -1;
    const int64_t c = r0 + n - 1, q = q0 + n - 1;
    if (c < pos1 - REGION - 1 || c >= pos1 + REGION + 1 || q >= L.l_seq) return -1;
    const uint32_t next = pile_u32(t, L.cigar + 4 * (int64_t)(k + 1)) & 15u;
    if (next != OP_I && next != OP_D) return -1;
    return lr_known(tens_base_code(t, L, q)) || tens_base_code(t, L, q) == 0 ? -1 : c;
}

// Does the record at text[off] (0-based start pos0) give the script's parser an entry at column c: a deleted base, or a matched one
// that is one of ACGTN?  (Serial; the hazards it is asked for are rare.)
LR_HD bool lr_entry_at(const uint8_t *t, int64_t len, int64_t off, int64_t pos0, int64_t c) {
    TensLayout L;
    if (!tens_layout(t, len, off, &L)) return false;
    int64_t rp = pos0, qp = 0;
    for (int32_t k = 0; k < L.n_cigar && rp <= c; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        const bool match = pile_is_match(op);
        if ((match || op == OP_D) && c < rp + (int64_t)n) {
            if (!match) return true;
            const int64_t q = qp + (c - rp);
            return q < L.l_seq && lr_known(tens_base_code(t, L, q));
        }
        if (match || op == OP_D || op == OP_N) rp += n;
        if (match || op == OP_I || op == OP_S) qp += n;
    }
    return false;
}

// cov and bad of a site -> its mask: a column exists iff it is covered and not bad; the walk of get_nearby_reads skips a missing
// column up to the centre and stops at the first one behind it
LR_HD void lr_finish_mask(const uint32_t *cov, const uint32_t *bad, uint32_t *mask) {
    for (int w = 0; w < WORDS; ++w) mask[w] = cov[w] & ~bad[w];
    int d = WINDOW + 1;
    while (d < COLS && ((mask[d >> 5] >> (d & 31)) & 1u)) ++d;
    for (; d < WORDS * 32; ++d) mask[d >> 5] &= ~(1u << (d & 31));
}

// Does the insertion at operation k show in the script's fragment?  The nearest operation before it that is not an I (nor an empty
// M, =, X or D) is a matched stretch -- a leading insertion, one behind a clip and one behind a deletion never appear -- and the
// nearest behind it that is not an I is not a D: mpileup spells `+2AA-3NNN` there and decode_pileup_bases keeps the deletion only.
LR_HD bool lr_ins_counts(const uint8_t *t, const TensLayout &L, int32_t k) {
    int32_t j = k - 1;
    bool before = false;
    for (; j >= 0; --j) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)j), op = w & 15u, n = w >> 4;
        if (op == OP_I || ((pile_is_match(op) || op == OP_D) && n == 0)) continue;
        before = pile_is_match(op);
        break;
    }
    if (!before) return false;
    for (j = k + 1; j < L.n_cigar; ++j) {
        const uint32_t op = pile_u32(t, L.cigar + 4 * (int64_t)j) & 15u;
        if (op == OP_I) continue;
        return op != OP_D;
    }
    return true;
}

// What operation k appends to the read's fragment over the surviving columns: emit(letter, column) once per byte, in order.
template <class Emit>
LR_HD int lr_frag_op(const uint8_t *t, const TensLayout &L, int32_t k, uint32_t op, int64_t n, int64_t r0, int64_t q0, int64_t w0,
                     const uint32_t *mask, Emit &emit) {
    if (pile_is_match(op)) {
        const int64_t a = r0 > w0 ? r0 : w0, b = r0 + n < w0 + COLS ? r0 + n : w0 + COLS;
        for (int64_t r = a; r < b; ++r) {
            if (!lr_bit(mask, r - w0)) continue;
            const int64_t q = q0 + (r - r0);
            if (q >= L.l_seq) return MPN_LR_PAST_BASES;
            const uint32_t code = tens_base_code(t, L, q);
            if (code == 0) return MPN_LR_EQ_BASE;
            if (lr_acgt(code)) emit(lr_letter(code), r);
        }
    } else if (op == OP_I && n > 0 && k < L.n_cigar && lr_bit(mask, r0 - 1 - w0) && lr_ins_counts(t, L, k)) {
        for (int64_t j = 0; j < n; ++j) {
            if (q0 + j >= L.l_seq) return MPN_LR_PAST_BASES;
            const uint32_t code = tens_base_code(t, L, q0 + j);
            if (code == 0) return MPN_LR_EQ_BASE;
            emit(lr_letter(code), r0 - 1);
        }
    }
    return MPN_LR_OK;
}

// ---- the serial walks: one record, one site --------------------------------------------------------------------------------------
struct LrPlainOr {
    uint32_t *cov, *bad;
    LR_HD void operator()(int word, uint32_t c, uint32_t b) { cov[word] |= c; bad[word] |= b; }
};

// adds the record at text[off] (0-based start pos0) to cov[WORDS] and bad[WORDS] of the site at pos1 -> MPN_LR_OK or why not
LR_HD int lr_cover_serial(const uint8_t *t, int64_t len, int64_t off, int64_t pos0, int64_t pos1, uint32_t *cov, uint32_t *bad) {
    TensLayout L;
    if (!tens_layout(t, len, off, &L)) return MPN_LR_PAST;
    if (L.l_seq == 0) return MPN_LR_NO_BASES;
    LrPlainOr orr{cov, bad};
    int64_t rp = pos0, qp = 0;
    for (int32_t k = 0; k < L.n_cigar && rp <= pos1 + REGION + 1; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        if (op > 8) return MPN_LR_BAD_OP;
        if (lr_skip_or_pad(op, n, rp, pos1)) return MPN_LR_SKIP_PAD;
        const int st = lr_cover_op(t, L, op, (int64_t)n, rp, qp, lr_w0(pos1), orr);
        if (st) return st;
        if (pile_is_match(op) || op == OP_D || op == OP_N) rp += n;
        if (pile_is_match(op) || op == OP_I || op == OP_S) qp += n;
    }
    return MPN_LR_OK;
}

// the hazard columns of the record at text[off] for the site at pos1: up to cap of them to cols -> their number (0 for a record that
// lr_cover_serial refuses)
LR_HD int lr_hazard_serial(const uint8_t *t, int64_t len, int64_t off, int64_t pos0, int64_t pos1, int64_t *cols, int cap) {
    TensLayout L;
    if (!tens_layout(t, len, off, &L)) return 0;
    int64_t rp = pos0, qp = 0;
    int found = 0;
    for (int32_t k = 0; k < L.n_cigar && rp <= pos1 + REGION + 1; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        if (op > 8) return found;
        const int64_t c = lr_hazard_op(t, L, k, op, (int64_t)n, rp, qp, pos1);
        if (c >= 0 && found < cap) cols[found++] = c;
        if (pile_is_match(op) || op == OP_D || op == OP_N) rp += n;
        if (pile_is_match(op) || op == OP_I || op == OP_S) qp += n;
    }
    return found;
}

struct LrPlainEmit {
    uint8_t *out;             // null: count only
    int64_t n, first;
    LR_HD void operator()(uint8_t letter, int64_t col) {
        if (n == 0) first = col;
        if (out) out[n] = letter;
        ++n;
    }
};

// the fragment of the record at text[off] over the mask of the site at pos1: *n bytes (to out unless null), *first its first column
LR_HD int lr_frag_serial(const uint8_t *t, int64_t len, int64_t off, int64_t pos0, int64_t pos1, const uint32_t *mask, uint8_t *out, int64_t *n,
                         int64_t *first) {
    TensLayout L;
    if (!tens_layout(t, len, off, &L)) return MPN_LR_PAST;
    if (L.l_seq == 0) return MPN_LR_NO_BASES;
    LrPlainEmit emit{out, 0, 0};
    int64_t rp = pos0, qp = 0;
    for (int32_t k = 0; k < L.n_cigar && rp <= pos1 + REGION + 1; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, cn = w >> 4;
        if (op > 8) return MPN_LR_BAD_OP;
        if (lr_skip_or_pad(op, cn, rp, pos1)) return MPN_LR_SKIP_PAD;
        const int st = lr_frag_op(t, L, k, op, (int64_t)cn, rp, qp, lr_w0(pos1), mask, emit);
        if (st) return st;
        if (pile_is_match(op) || op == OP_D || op == OP_N) rp += cn;
        if (pile_is_match(op) || op == OP_I || op == OP_S) qp += cn;
    }
    *n = emit.n;
    *first = emit.first;
    return MPN_LR_OK;
}

// ---- alleles ---------------------------------------------------------------------------------------------------------------------
// A key before its text.  kind 0: the fragment's letter at off; 1: 'I' and len letters of the fragment arena from off; 2: 'D' and
// len bytes of the contig from off, upper-cased.
struct LrKeyRef { int32_t kind, len; int64_t off; };

LR_HD int32_t lr_key_strlen(const LrKeyRef &k) { return k.len + (k.kind ? 1 : 0); }
LR_HD uint8_t lr_key_char(const LrKeyRef &k, int32_t i, const uint8_t *letters, const uint8_t *contig) {
    if (k.kind) {
        if (i == 0) return k.kind == 1 ? 'I' : 'D';
        --i;
    }
    return k.kind == 2 ? lr_upper(contig[k.off + i]) : letters[k.off + i];
}
LR_HD bool lr_key_equal(const LrKeyRef &a, const LrKeyRef &b, const uint8_t *letters, const uint8_t *contig) {
    const int32_t n = lr_key_strlen(a);
    if (n != lr_key_strlen(b)) return false;
    for (int32_t i = 0; i < n; ++i)
        if (lr_key_char(a, i, letters, contig) != lr_key_char(b, i, letters, contig)) return false;
    return true;
}

// The keys that the script counts for one read of the site at pos1, from its SSW result (score > 0) and CIGAR (M, I, D as ssw.c
// writes them): pyssw spells a clip of read_begin1 in front and one of frag_len - (read_end1 - read_begin1 + 1) behind; the script
// cuts the latter off the fragment, drops both from the CIGAR and walks from query index 0 -- the shift by the leading clip is
// the script's and is kept.  -> the number of keys (at most MAX_KEYS, in the order of the walk); *ref_pos = where the walk starts.
LR_HD int lr_pair_keys(int32_t ref_begin1, int32_t read_begin1, int32_t read_end1, const uint32_t *cig, int32_t cig_len, int64_t frag_off,
                       int32_t frag_len, int64_t pos1, int64_t contig_len, LrKeyRef *keys, int64_t *ref_pos) {
    int64_t clip_end = (int64_t)frag_len - ((int64_t)read_end1 - read_begin1 + 1);
    if (clip_end < 0) clip_end = 0;
    const int64_t seq_len = frag_len - clip_end;
    int64_t r = (int64_t)ref_begin1 + pos1 - FLANK_REF, q = 0;      // 1-based
    *ref_pos = r;
    int n_keys = 0;
    for (int32_t k = 0; k < cig_len; ++k) {
        const uint32_t op = cig[k] & 15u;
        const int64_t n = cig[k] >> 4;
        if (op == 1) {
            if (pos1 == r - 1 && n_keys < MAX_KEYS) {
                const int64_t a = q < seq_len ? q : seq_len, b = q + n < seq_len ? q + n : seq_len;
                keys[n_keys++] = LrKeyRef{1, (int32_t)(b - a), frag_off + a};
            }
            q += n;
        } else if (op == 2) {
            if (pos1 == r - 1 && n_keys < MAX_KEYS) {
                int64_t a = r - 1, b = r - 1 + n;
                if (a > contig_len) a = contig_len;
                if (b > contig_len) b = contig_len;
                keys[n_keys++] = LrKeyRef{2, (int32_t)(b - a), a};
            }
            r += n;
        } else {                                                    // M (0; ssw.c writes no = or X), read as `=`
            if (pos1 >= r && r + n > pos1 && q + pos1 - r < seq_len && n_keys < MAX_KEYS) keys[n_keys++] = LrKeyRef{0, 1, frag_off + q + pos1 - r};
            r += n;
            q += n;
        }
    }
    return n_keys;
}

}  // namespace mpn_lr

#include <queue>
#include <vector>
namespace mpn_lr {
// samtools' -d: walking the candidates of a site in file order (start ascending; end exclusive), one is dropped iff it is not the
// first of its start and at least maxcnt kept ones have end >= its start.
inline void lr_depth_rule(int64_t n, const int64_t *start, const int64_t *end, int32_t maxcnt, uint8_t *keep) {
    std::priority_queue<int64_t, std::vector<int64_t>, std::greater<int64_t>> alive;      // the ends of the kept ones, smallest on top
    for (int64_t i = 0; i < n; ++i) {
        const bool first = i == 0 || start[i] != start[i - 1];
        while (!alive.empty() && alive.top() < start[i]) alive.pop();
        keep[i] = first || (int64_t)alive.size() < maxcnt;
        if (keep[i]) alive.push(end[i]);
    }
}
}  // namespace mpn_lr
