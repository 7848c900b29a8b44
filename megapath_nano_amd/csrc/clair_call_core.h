// The arithmetic and index maps behind include/mpn_call.h that are the same on the device and on the host: which reads form a
// site's pile-up column (call_taken, call_in_column), the indel event a read shows there (call_event_at, after htslib's
// resolve_cigar2 and samtools' pileup_seq), the events of a site taken serially (call_site_serial: the host check and the statement
// of what the wave of call_indels_kernel computes), and the decoding of one site (call_decode, after output_from / output_with of
// clair/call_var.py as DESIGN.md section 6 item 19 restates them).  call_decode is written once over a `Par`: the lanes that share
// the work and their reductions; CallSerial is one lane (scripts/clair_call_host_check.cpp), the kernel gives a wave.
//
// Bounds: as in tensor_core.h; a CIGAR operation is read only at an index below n_cigar, a base only at a query index below
// l_seq, a byte of the contig only inside [0, contig_len), of a reference string only below its length.
#pragma once
#include <stdint.h>
#include "../../include/mpn_call.h"
#include "tensor_core.h"

#define CALL_HD TENS_HD

namespace mpn_call {

using namespace mpn_tens;

constexpr int MAXLEN = MPN_CALL_MAX_LEN, VL = 16;

// one float32 multiply, rounded once (no contraction into a fused multiply-add)
CALL_HD float call_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    volatile float r = a * b;
    return r;
#endif
}
CALL_HD float call_max(float a, float b) { return b > a ? b : a; }        // Python's max(a, b)

// ---- the column --------------------------------------------------------------------------------------------------------------
// c: the 0-based column (site - 1).  The pile-up is asked for the base behind it.
CALL_HD bool call_taken(int64_t pos, int64_t rlen, int64_t c) { return pos <= c + 1 && pos + (rlen > 0 ? rlen : 1) > c + 1; }
CALL_HD bool call_in_column(int64_t pos, int64_t rlen, int64_t c) { return pos <= c && c < pos + rlen; }

struct CallEvent {
    int32_t kind;              // -1: none
    int32_t len;
    int32_t bad;               // 1: a base that does not exist
    int32_t del_len;           // an insertion: the deletion right behind it, which the pile-up spells into the same text (else 0)
    int32_t key_len;           // the bytes of the key in bases: an insertion's text behind the number; -1: longer than MAXLEN
    uint8_t bases[MAXLEN];
};

CALL_HD uint8_t call_base_char(uint32_t code) {
    const char s[17] = "=ACMGRSVTWYHKDBN";
    return (uint8_t)s[code & 15u];
}

// The event of a read at column c, whose operation k (code op: M, =, X, D or N; length n; from reference position r0 and query
// index q0) covers c.  resolve_cigar2: only the last position of an operation looks at the next one.
CALL_HD void call_event_at(const uint8_t *t, const TensLayout &L, int32_t k, uint32_t op, int64_t n, int64_t r0, int64_t q0, int64_t c, CallEvent *ev) {
    ev->kind = -1; ev->len = 0; ev->bad = 0; ev->del_len = 0; ev->key_len = 0;
    if (r0 + n - 1 != c || k + 1 >= L.n_cigar) return;
    const int is_del = pile_is_match(op) ? 0 : 1;
    const int64_t qpos = is_del ? q0 : q0 + (c - r0);
    const uint32_t w2 = pile_u32(t, L.cigar + 4 * (int64_t)(k + 1)), op2 = w2 & 15u, l2 = w2 >> 4;
    if (op2 == OP_D) {
        if (l2 >= 1 && l2 <= (uint32_t)MAXLEN) { ev->kind = MPN_CALL_DELETION; ev->len = (int32_t)l2; ev->key_len = (int32_t)l2; }
        return;
    }
    bool ins = op2 == OP_I && l2 > 0;
    if (op2 == OP_P && k + 2 < L.n_cigar) {              // a pad: the insertions behind it, up to the next M, D, N, = or X
        for (int32_t j = k + 2; j < L.n_cigar; ++j) {
            const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)j), o = w & 15u;
            if (o == OP_I && (w >> 4) > 0) ins = true;
            else if (o == OP_D || o == OP_N || pile_is_match(o)) break;
        }
    }
    if (!ins) return;
    // bam_plp_insertion: the run of insertions and pads behind k; a deletion right behind it is spelled into the same text
    int64_t total = 0, deletion = 0;
    int32_t stop = k + 1;
    for (; stop < L.n_cigar; ++stop) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)stop), o = w & 15u;
        if (o != OP_P && o != OP_I) { deletion = o == OP_D ? (int64_t)(w >> 4) : 0; break; }
        total += w >> 4;
    }
    if (total > MAXLEN) return;                          // can never be selected
    bool past = false;
    int64_t at = 0, j = 1;
    for (int32_t i = k + 1; i < stop; ++i) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)i), o = w & 15u, l = w >> 4;
        for (uint32_t x = 0; x < l; ++x) {
            if (o == OP_P) { ev->bases[at++] = '*'; continue; }
            const int64_t q = qpos + j++ - is_del;
            if (q < 0 || q >= L.l_seq) { past = true; ev->bases[at++] = 'N'; continue; }
            ev->bases[at++] = call_base_char(tens_base_code(t, L, q));
        }
    }
    if (past) { ev->bad = 1; return; }
    ev->kind = MPN_CALL_INSERTION;
    ev->len = (int32_t)total;
    ev->key_len = (int32_t)total;
    if (deletion > 0) {                                    // `+2AA-3NNN`: the script takes `AA-3NNN` for the inserted bases
        ev->del_len = (int32_t)deletion;
        const int64_t all = total + 1 + tens_digits((uint32_t)deletion) + deletion;
        if (all > MAXLEN) { ev->key_len = -1; return; }
        ev->bases[at++] = '-';
        at += tens_put(ev->bases, at, MAXLEN, (uint32_t)deletion);
        for (int64_t i = 0; i < deletion; ++i) ev->bases[at++] = 'N';
        ev->key_len = (int32_t)all;
    }
}

// The event of the record at text[off] at column c, on one thread.  Returns 0, or 1 for a record that does not lie inside the
// text or has an operation code above 8.
CALL_HD int call_event_serial(const uint8_t *t, int64_t len, int64_t off, int64_t pos, int64_t c, CallEvent *ev) {
    ev->kind = -1; ev->len = 0; ev->bad = 0; ev->del_len = 0; ev->key_len = 0;
    TensLayout L;
    if (!tens_layout(t, len, off, &L)) return 1;
    int64_t rp = pos, qp = 0;
    for (int32_t k = 0; k < L.n_cigar && rp <= c; ++k) {
        const uint32_t w = pile_u32(t, L.cigar + 4 * (int64_t)k), op = w & 15u, n = w >> 4;
        if (op > 8) return 1;
        const bool on_ref = pile_is_match(op) || op == OP_D || op == OP_N;
        if (on_ref && rp <= c && c < rp + (int64_t)n) {
            call_event_at(t, L, k, op, (int64_t)n, rp, qp, c, ev);
            return 0;
        }
        if (on_ref) rp += n;
        if (pile_is_match(op) || op == OP_I || op == OP_S) qp += n;
    }
    return 0;
}

CALL_HD bool call_same_event(const mpn_call_event &e, const uint8_t *e_bases, const CallEvent &v) {
    if (e.kind != v.kind || e.len != v.len || (v.kind == MPN_CALL_INSERTION && e.clip != v.del_len)) return false;
    if (v.kind == MPN_CALL_INSERTION)
        for (int i = 0; i < v.len; ++i)
            if (e_bases[i] != v.bases[i]) return false;
    return true;
}
CALL_HD int call_stored(const CallEvent &v) { return v.key_len < 0 ? v.len : v.key_len; }      // the bytes of v.bases that are set
CALL_HD int32_t call_clip(int32_t n, int64_t site, int64_t contig_len) {     // len(fasta.fetch(start=site, end=site + n))
    const int64_t room = contig_len - site;
    return (int32_t)(room <= 0 ? 0 : ((int64_t)n < room ? (int64_t)n : room));
}

// The events of one site over reads[begin .. end), serially: ev[0 .. *n_ev) and their bases (MAXLEN each) in the order of first
// appearance.  Returns 0; 1: *bad = the first bad read; 2: more than cap events.
CALL_HD int call_site_serial(const uint8_t *t, int64_t len, const mpn_call_read *reads, int64_t begin, int64_t end, int64_t site, int64_t contig_len,
                             mpn_call_event *ev, uint8_t *bases, int32_t cap, int32_t *n_ev, int64_t *bad) {
    const int64_t c = site - 1;
    int64_t taken = 0, last_pos = -1;
    int32_t rank = 0;
    bool any = false;
    *n_ev = 0;
    for (int64_t r = begin; r < end; ++r) {
        const mpn_call_read &rd = reads[r];
        if (!call_taken(rd.pos, rd.rlen, c)) continue;
        const bool first = !any || rd.pos != last_pos, kept = taken < MPN_CALL_MAX_DEPTH || first;
        any = true; last_pos = rd.pos; ++taken;
        if (!kept || !call_in_column(rd.pos, rd.rlen, c)) continue;
        CallEvent v;
        if (call_event_serial(t, len, rd.off, rd.pos, c, &v) || v.bad) { *bad = r; return 1; }
        const int32_t my_rank = rank++;
        if (v.kind < 0) continue;
        int32_t e = 0;
        for (; e < *n_ev; ++e)
            if (call_same_event(ev[e], bases + (int64_t)e * MAXLEN, v)) break;
        if (e < *n_ev) { ++ev[e].count; continue; }
        if (e >= cap) return 2;
        ev[e].kind = v.kind; ev[e].len = v.len; ev[e].count = 1; ev[e].rank = my_rank; ev[e].bases = 0;
        ev[e].clip = v.kind == MPN_CALL_DELETION ? call_clip(v.len, site, contig_len) : v.del_len;
        ev[e].key_len = v.kind == MPN_CALL_DELETION ? ev[e].clip : v.key_len;
        for (int i = 0; i < MAXLEN; ++i) bases[(int64_t)e * MAXLEN + i] = v.kind == MPN_CALL_INSERTION && i < call_stored(v) ? v.bases[i] : 0;
        ++*n_ev;
    }
    return 0;
}

// ---- the outcomes --------------------------------------------------------------------------------------------------------------
// The lists of possible_outcome_probabilites_from, one behind the other, each in the order the script builds it.
enum { L_REF = 0, L_HOMO_SNP, L_HET_SNP, L_HOMO_INS, L_ACGT_INS, L_INS_INS, L_HOMO_DEL, L_ACGT_DEL, L_DEL_DEL, L_INS_DEL, N_LISTS };
constexpr int AT_REF = 0, AT_HOMO_SNP = 1, AT_HET_SNP = 5, AT_HOMO_INS = 11, AT_ACGT_INS = 27, AT_INS_INS = 91, AT_HOMO_DEL = 347, AT_ACGT_DEL = 363,
              AT_DEL_DEL = 427, AT_INS_DEL = 667, N_VALUES = 1179;
constexpr int G21_DELDEL = 10, G21_ADEL = 11, G21_INSINS = 15, G21_AINS = 16, G21_INSDEL = 20;

CALL_HD int call_list_of(int i) {
    return i < AT_HOMO_SNP ? L_REF : i < AT_HET_SNP ? L_HOMO_SNP : i < AT_HOMO_INS ? L_HET_SNP : i < AT_ACGT_INS ? L_HOMO_INS : i < AT_INS_INS ? L_ACGT_INS :
           i < AT_HOMO_DEL ? L_INS_INS : i < AT_ACGT_DEL ? L_HOMO_DEL : i < AT_DEL_DEL ? L_ACGT_DEL : i < AT_INS_DEL ? L_DEL_DEL : L_INS_DEL;
}
CALL_HD int call_homo_gt21(int k) { const int g[4] = {0, 4, 7, 9}; return g[k]; }
CALL_HD int call_het_gt21(int k) { const int g[6] = {1, 2, 3, 5, 6, 8}; return g[k]; }
// the second index of entry jj (0 .. 14) of row i of the two-deletion list, which leaves j == i out
CALL_HD int call_deldel_j(int i, int jj) { return jj + 1 + (jj + 1 >= i ? 1 : 0); }

// value i of the lists.  pr: the 90 probabilities; ref_gt21: the gt21 of the reference base twice.  Every product is formed left
// to right as numpy's float32 scalars form it.
CALL_HD float call_value(int i, const float *pr, int ref_gt21) {
    const float *gt = pr, *g = pr + 21, *v1 = pr + 24 + VL, *v2 = pr + 57 + VL;      // v1[k], v2[k]: length k, -16 .. 16
    const float vl0 = call_mul(v1[0], v2[0]);
    if (i < AT_HOMO_SNP) return call_mul(call_mul(vl0, g[0]), gt[ref_gt21]);
    if (i < AT_HET_SNP) return call_mul(call_mul(vl0, g[1]), gt[call_homo_gt21(i - AT_HOMO_SNP)]);
    if (i < AT_HOMO_INS) return call_mul(call_mul(vl0, g[2]), gt[call_het_gt21(i - AT_HET_SNP)]);
    if (i < AT_ACGT_INS) { const int k = i - AT_HOMO_INS + 1; return call_mul(call_mul(v1[k], v2[k]), call_mul(g[1], gt[G21_INSINS])); }
    if (i < AT_INS_INS) {
        const int k = (i - AT_ACGT_INS) / 4 + 1, b = (i - AT_ACGT_INS) % 4;
        return call_mul(call_mul(call_max(call_mul(v1[0], v2[k]), call_mul(v1[k], v2[0])), gt[G21_AINS + b]), g[2]);
    }
    if (i < AT_HOMO_DEL) {
        const int a = (i - AT_INS_INS) / 16 + 1, b = (i - AT_INS_INS) % 16 + 1;
        return call_mul(call_mul(v1[a], v2[b]), call_mul(g[2], gt[G21_INSINS]));
    }
    if (i < AT_ACGT_DEL) { const int k = i - AT_HOMO_DEL + 1; return call_mul(call_mul(v1[-k], v2[-k]), call_mul(g[1], gt[G21_DELDEL])); }
    if (i < AT_DEL_DEL) {
        const int k = (i - AT_ACGT_DEL) / 4 + 1, b = (i - AT_ACGT_DEL) % 4;
        return call_mul(call_mul(call_max(call_mul(v1[0], v2[-k]), call_mul(v1[-k], v2[0])), gt[G21_ADEL + b]), g[2]);
    }
    if (i < AT_INS_DEL) {
        const int a = (i - AT_DEL_DEL) / 15 + 1, b = call_deldel_j(a, (i - AT_DEL_DEL) % 15);
        return call_mul(call_mul(v1[-a], v2[-b]), call_mul(g[2], gt[G21_DELDEL]));
    }
    const int e = (i - AT_INS_DEL) & 1, a = ((i - AT_INS_DEL) >> 1) / 16 + 1, b = ((i - AT_INS_DEL) >> 1) % 16 + 1;
    const float extra = call_mul(g[2], gt[G21_INSDEL]);
    return e == 0 ? call_mul(call_mul(v1[a], v2[-b]), extra) : call_mul(call_mul(v1[-a], v2[b]), extra);
}

CALL_HD int call_base_num(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : (b == 'T' || b == 'U') ? 3 : -1; }

// one lane that does everything
struct CallSerial {
    CALL_HD int lane() const { return 0; }
    CALL_HD int lanes() const { return 1; }
    CALL_HD float max_f(float v) const { return v; }
    CALL_HD int min_i(int v) const { return v; }
    CALL_HD long long max_ll(long long v) const { return v; }
    CALL_HD int or_i(int v) const { return v; }
    CALL_HD void sync() const {}
};

struct CallSite {
    const float *probs;            // 90
    const int32_t *x;              // 1056
    const uint8_t *ref;            // the reference string
    int32_t ref_n;                 // 17 .. 33
    const uint8_t *contig;
    int64_t contig_len;
    int64_t site;                  // 1-based
    const mpn_call_event *ev;
    const uint8_t *bases;          // MAXLEN per event
    int32_t n_ev;
    int32_t options;
};

// What the lanes share of one site: the values, the alleles, and the strings in the making.  (Every lane writes the same bytes.)
struct CallWork {
    float vals[N_VALUES];
    uint8_t alleles[MPN_CALL_ALLELE_BYTES];
    uint8_t ins[MAXLEN], ins2[MAXLEN], del[MAXLEN];
};

CALL_HD int32_t call_cell(const CallSite &S, int index, int row, int channel) { return S.x[(index * ROWS + row) * CHANNELS + channel]; }
CALL_HD int32_t call_sum(const CallSite &S, int index, int channel) {
    int32_t s = 0;
    for (int r = 0; r < ROWS; ++r) s += call_cell(S, index, r, channel);
    return s;
}

// insertion_bases_using_pysam_from / deletion_bases_using_pysam_from over the site's events: the best count of the events of
// `kind` with a length in [mn, mx] that are not `ignore`, the first to appear among equals.  A deletion's key is its clipped
// length: the events that share it count together.  -> the event, or -1.
template <class Par>
CALL_HD int call_lookup(const Par &par, const CallSite &S, int kind, int mn, int mx, const uint8_t *ignore, int ignore_len) {
    long long best = -1;
    for (int e = par.lane(); e < S.n_ev; e += par.lanes()) {
        const mpn_call_event &E = S.ev[e];
        if (E.kind != kind || E.len < mn || E.len > mx) continue;
        long long total = E.count, rank = E.rank;
        if (kind == MPN_CALL_INSERTION) {
            if (ignore && E.key_len == ignore_len) {
                bool same = true;
                for (int i = 0; i < E.key_len; ++i) same = same && S.bases[(int64_t)e * MAXLEN + i] == ignore[i];
                if (same) continue;
            }
        } else {
            for (int o = 0; o < S.n_ev; ++o) {
                const mpn_call_event &O = S.ev[o];
                if (o == e || O.kind != kind || O.len < mn || O.len > mx || O.clip != E.clip) continue;
                total += O.count;
                if (O.rank < rank) rank = O.rank;
            }
        }
        const long long key = (total << 40) | ((0xfffffffLL - rank) << 12) | (long long)(0xfff - e);
        if (key > best) best = key;
    }
    best = par.max_ll(best);
    return best < 0 ? -1 : 0xfff - (int)(best & 0xfff);
}

// the tensor's opinion on the inserted base at index `at`: argmax([v0, v1, v2, v3, 0, 0, 0, 0]) % 4, the first maximum; *sum_out:
// the sum of the four
CALL_HD uint8_t call_tensor_base(const CallSite &S, int at, int32_t *sum_out) {
    int32_t v[4], sum = 0;
    for (int b = 0; b < 4; ++b) {
        v[b] = call_cell(S, at, b, 1) + call_cell(S, at, b + 4, 1) - (call_cell(S, at, b, 3) + call_cell(S, at, b + 4, 3));
        sum += v[b];
    }
    int arg = 0;
    for (int b = 1; b < 4; ++b) if (v[b] > v[arg]) arg = b;
    if (0 > v[arg]) arg = 4;
    if (sum_out) *sum_out = sum;
    const char s[5] = "ACGT";
    return (uint8_t)s[arg % 4];
}

// insertion_bases_from -> the length; the bases in out.  -1: the key of the chosen event is longer than MAXLEN
template <class Par>
CALL_HD int call_insertion(const Par &par, const CallSite &S, int v, uint8_t *out) {
    const bool all = (S.options & MPN_CALL_PYSAM_ALL) != 0;
    if (!all && v < VL) {
        for (int i = 0; i < v; ++i) out[i] = call_tensor_base(S, FLANK + 1 + i, nullptr);
        return v;
    }
    const int e = call_lookup(par, S, MPN_CALL_INSERTION, v, v >= VL ? MAXLEN : v, nullptr, 0);
    if (e >= 0) {
        const int n = S.ev[e].key_len;
        for (int i = 0; i < n; ++i) out[i] = S.bases[(int64_t)e * MAXLEN + i];
        return n;
    }
    if (all) return 0;
    int n = 0;                                               // inferred_insertion_bases_from
    for (int at = FLANK + 1; at < 2 * FLANK + 1; ++at) {
        int32_t sum = 0;
        const uint8_t b = call_tensor_base(S, at, &sum);
        if (at < FLANK + VL || 8 * (int64_t)sum >= (int64_t)call_sum(S, at, 0)) out[n++] = b;
        else break;
    }
    return n;
}

// deletion_bases_from -> the length; the bases in out
template <class Par>
CALL_HD int call_deletion(const Par &par, const CallSite &S, int v, uint8_t *out) {
    const bool all = (S.options & MPN_CALL_PYSAM_ALL) != 0;
    int n = 0;
    if (all || v >= VL) {
        const int e = call_lookup(par, S, MPN_CALL_DELETION, v, v >= VL ? MAXLEN : v, nullptr, 0);
        if (e >= 0) {
            n = S.ev[e].clip;
            for (int i = 0; i < n; ++i) {
                const int64_t at = S.site + i;
                out[i] = at >= 0 && at < S.contig_len ? S.contig[at] : (uint8_t)'N';
            }
        }
        if (all || n >= FLANK) return n;
    }
    n = S.ref_n - (FLANK + 1);
    n = n < 0 ? 0 : (n < v ? n : v);
    for (int i = 0; i < n; ++i) out[i] = S.ref[FLANK + 1 + i];
    return n;
}

CALL_HD int call_put(uint8_t *to, int at, const uint8_t *from, int n) {
    for (int i = 0; i < n; ++i) to[at + i] = from[i];
    return at + n;
}
CALL_HD bool call_equal(const uint8_t *a, int na, const uint8_t *b, int nb) {
    if (na != nb) return false;
    for (int i = 0; i < na; ++i) if (a[i] != b[i]) return false;
    return true;
}
// partial_label_from: 'D', 'I', or the first byte of the alternate
CALL_HD int call_partial(int ref_len, const uint8_t *alt, int alt_len) { return ref_len > alt_len ? 256 : ref_len < alt_len ? 257 : alt[0]; }
// mix_two_partial_labels -> the gt21, or -1 where the script raises
CALL_HD int call_mix(int a, int b) {
    if (a < 256 && b < 256) {
        int x = call_base_num((uint8_t)a), y = call_base_num((uint8_t)b);
        if (a == 'U' || b == 'U' || x < 0 || y < 0) return -1;
        if (x > y) { const int s = x; x = y; y = s; }
        const int first[4] = {0, 4, 7, 9};
        return first[x] + (y - x);
    }
    if (a < 256 || b < 256) {
        const int base = a < 256 ? a : b, other = a < 256 ? b : a, x = call_base_num((uint8_t)base);
        if (base == 'U' || x < 0) return -1;
        return (other == 256 ? G21_ADEL : G21_AINS) + x;
    }
    return a == b ? (a == 256 ? G21_DELDEL : G21_INSINS) : G21_INSDEL;
}

// One site: output_with up to the numbers of the line.  -> the status; for MPN_CALL_EMITTED the row (its site is the caller's)
// and W->alleles are filled.  Every lane of par runs this with the same arguments and gets the same answer.
template <class Par>
CALL_HD int call_decode(const Par &par, const CallSite &S, CallWork *W, mpn_call_row *row) {
    int bad = 0;
    for (int i = par.lane(); i < MPN_CALL_PROBS; i += par.lanes()) {
        const float p = S.probs[i];
        if (!(p >= 0.0f) || !(p <= 3.0e38f)) bad = 1;
    }
    if (par.or_i(bad)) return MPN_CALL_BAD_PROB;
    const uint8_t centre = S.ref[FLANK];
    if (!(centre == 'A' || centre == 'C' || centre == 'G' || centre == 'T' || centre == 'U')) return MPN_CALL_NOT_ACGT;
    const int32_t depth = call_sum(S, FLANK, 2) + call_sum(S, FLANK, 0);
    if (depth == 0) return MPN_CALL_NO_DEPTH;
    const uint8_t centre_acgt = centre == 'U' ? (uint8_t)'T' : centre;
    const int ref_gt21 = call_homo_gt21(call_base_num(centre_acgt));
    for (int i = par.lane(); i < N_VALUES; i += par.lanes()) W->vals[i] = call_value(i, S.probs, ref_gt21);
    par.sync();
    uint8_t *REF = W->alleles, *ALT1 = W->alleles + MPN_CALL_ALT1_AT, *ALT2 = W->alleles + MPN_CALL_ALT2_AT;
    int ref_len = 0, alt1_len = 0, alt2_len = 0, flags = 0;
    const float *gt = S.probs, *g = S.probs + 21;
    const char acgt[5] = "ACGT";
    for (;;) {
        float mx = 0.0f;
        for (int i = par.lane(); i < N_VALUES; i += par.lanes()) mx = call_max(mx, W->vals[i]);
        mx = par.max_f(mx);
        int first[N_LISTS];
        for (int l = 0; l < N_LISTS; ++l) first[l] = 0x7fffffff;
        for (int i = par.lane(); i < N_VALUES; i += par.lanes())
            if (W->vals[i] == mx) {
                const int l = call_list_of(i);
                if (i < first[l]) first[l] = i;
            }
        flags = 0;
        for (int l = 0; l < N_LISTS; ++l) {
            first[l] = par.min_i(first[l]);
            if (first[l] != 0x7fffffff) flags |= 1 << l;
        }
        const int hetero = (1 << L_HET_SNP) | (1 << L_ACGT_INS) | (1 << L_INS_INS) | (1 << L_ACGT_DEL) | (1 << L_DEL_DEL) | (1 << L_INS_DEL);
        if ((flags & 1) || ((S.options & MPN_CALL_HAPLOID) && (flags & hetero))) {
            flags = 1;
            REF[0] = ALT1[0] = centre_acgt;
            ref_len = alt1_len = 1; alt2_len = 0;
            break;
        }
        par.sync();                                           // (the values are read before one of them is taken out)
        if (flags & (1 << L_HOMO_SNP)) {
            int k = 0;
            for (int i = 1; i < 4; ++i) if (gt[call_homo_gt21(i)] > gt[call_homo_gt21(k)]) k = i;
            REF[0] = centre; ALT1[0] = (uint8_t)acgt[k];
            ref_len = alt1_len = 1; alt2_len = 0;
            break;
        }
        if (flags & (1 << L_HET_SNP)) {
            int k = 0;
            for (int i = 1; i < 6; ++i) if (gt[call_het_gt21(i)] > gt[call_het_gt21(k)]) k = i;
            const char l1[7] = "AAACCG", l2[7] = "CGTGTT";
            const uint8_t b1 = (uint8_t)l1[k], b2 = (uint8_t)l2[k];
            REF[0] = centre; ref_len = 1;
            if (b1 != centre && b2 != centre) { ALT1[0] = b1; ALT2[0] = b2; alt1_len = alt2_len = 1; }
            else { ALT1[0] = b1 != centre ? b1 : b2; alt1_len = 1; alt2_len = 0; }
            break;
        }
        if (flags & (1 << L_HOMO_INS)) {
            const int idx = first[L_HOMO_INS], v = idx - AT_HOMO_INS + 1;
            W->vals[idx] = -1.0f;
            const int n = call_insertion(par, S, v, W->ins);
            if (n < 0) return MPN_CALL_LONG_KEY;
            if (n == 0) { par.sync(); continue; }
            REF[0] = centre; ref_len = 1;
            ALT1[0] = centre; alt1_len = call_put(ALT1, 1, W->ins, n); alt2_len = 0;
            break;
        }
        if (flags & (1 << L_ACGT_INS)) {
            const int idx = first[L_ACGT_INS], v = (idx - AT_ACGT_INS) / 4 + 1;
            const uint8_t b = (uint8_t)acgt[(idx - AT_ACGT_INS) % 4];
            W->vals[idx] = -1.0f;
            const int n = call_insertion(par, S, v, W->ins);
            if (n < 0) return MPN_CALL_LONG_KEY;
            if (n == 0) { par.sync(); continue; }
            REF[0] = centre; ref_len = 1;
            if (b != centre) {
                ALT1[0] = b; alt1_len = 1;
                ALT2[0] = centre; alt2_len = call_put(ALT2, 1, W->ins, n);
            } else {
                ALT1[0] = centre; alt1_len = call_put(ALT1, 1, W->ins, n); alt2_len = 0;
            }
            break;
        }
        if (flags & (1 << L_INS_INS)) {
            const int idx = first[L_INS_INS], a = (idx - AT_INS_INS) / 16 + 1, b = (idx - AT_INS_INS) % 16 + 1, v1 = a <= b ? a : b, v2 = a <= b ? b : a;
            W->vals[idx] = -1.0f;
            const int n = call_insertion(par, S, v2, W->ins);
            if (n < 0) return MPN_CALL_LONG_KEY;
            if (n == 0) { par.sync(); continue; }
            const int e = call_lookup(par, S, MPN_CALL_INSERTION, v1, v1 >= VL ? MAXLEN : v1, W->ins, n);
            int n2;
            if (e >= 0) {
                n2 = S.ev[e].key_len;
                if (n2 < 0) return MPN_CALL_LONG_KEY;
                for (int i = 0; i < n2; ++i) W->ins2[i] = S.bases[(int64_t)e * MAXLEN + i];
            } else {
                n2 = n < v1 ? n : v1;
                for (int i = 0; i < n2; ++i) W->ins2[i] = W->ins[i];
            }
            if (call_equal(W->ins, n, W->ins2, n2)) { par.sync(); continue; }
            REF[0] = centre; ref_len = 1;
            ALT1[0] = centre; alt1_len = call_put(ALT1, 1, W->ins2, n2);
            ALT2[0] = centre; alt2_len = call_put(ALT2, 1, W->ins, n);
            break;
        }
        if (flags & (1 << L_HOMO_DEL)) {
            const int idx = first[L_HOMO_DEL], v = idx - AT_HOMO_DEL + 1;
            W->vals[idx] = -1.0f;
            const int n = call_deletion(par, S, v, W->del);
            if (n == 0) { par.sync(); continue; }
            REF[0] = centre; ref_len = call_put(REF, 1, W->del, n);
            ALT1[0] = centre; alt1_len = 1; alt2_len = 0;
            break;
        }
        if (flags & (1 << L_ACGT_DEL)) {
            const int idx = first[L_ACGT_DEL], v = (idx - AT_ACGT_DEL) / 4 + 1;
            const uint8_t b = (uint8_t)acgt[(idx - AT_ACGT_DEL) % 4];
            W->vals[idx] = -1.0f;
            const int n = call_deletion(par, S, v, W->del);
            if (n == 0) { par.sync(); continue; }
            REF[0] = centre; ref_len = call_put(REF, 1, W->del, n);
            ALT1[0] = centre; alt1_len = 1; alt2_len = 0;
            if (b != centre) { ALT2[0] = b; alt2_len = call_put(ALT2, 1, W->del, n); }
            break;
        }
        if (flags & (1 << L_DEL_DEL)) {
            const int idx = first[L_DEL_DEL], a = (idx - AT_DEL_DEL) / 15 + 1, b = call_deldel_j(a, (idx - AT_DEL_DEL) % 15), v1 = a < b ? a : b,
                      v2 = a < b ? b : a;
            W->vals[idx] = -1.0f;
            const int n = call_deletion(par, S, v2, W->del);
            if (n == 0 || n <= v1) { par.sync(); continue; }           // (n <= v1: both alternates would be the centre alone)
            REF[0] = centre; ref_len = call_put(REF, 1, W->del, n);
            ALT1[0] = centre; alt1_len = 1;
            ALT2[0] = centre; alt2_len = call_put(ALT2, 1, W->del + v1, n - v1);
            break;
        }
        {
            const int idx = first[L_INS_DEL], e = (idx - AT_INS_DEL) & 1, a = ((idx - AT_INS_DEL) >> 1) / 16 + 1, b = ((idx - AT_INS_DEL) >> 1) % 16 + 1,
                      v1 = e == 0 ? b : a, v2 = e == 0 ? a : b;
            W->vals[idx] = -1.0f;
            const int ni = call_insertion(par, S, v2, W->ins), nd = call_deletion(par, S, v1, W->del);
            if (ni < 0) return MPN_CALL_LONG_KEY;
            if (ni == 0 || nd == 0) { par.sync(); continue; }
            REF[0] = centre; ref_len = call_put(REF, 1, W->del, nd);
            ALT1[0] = centre; alt1_len = 1;
            ALT2[0] = centre; alt2_len = call_put(ALT2, call_put(ALT2, 1, W->ins, ni), W->del, nd);
            break;
        }
    }
    const bool is_ref = (flags & 1) != 0, multi = alt2_len > 0;
    if (is_ref && !(S.options & MPN_CALL_SHOW_REF)) return MPN_CALL_REFERENCE;
    if (!is_ref && !multi && call_equal(REF, ref_len, ALT1, alt1_len)) return MPN_CALL_SAME;
    int genotype = 3;
    if (!multi) genotype = is_ref ? 0 : (flags & ((1 << L_HOMO_SNP) | (1 << L_HOMO_INS) | (1 << L_HOMO_DEL))) ? 1 : 2;
    // supported reads, in output_with's own order of the flags
    const auto snp = [&](uint8_t base, int *wrong) -> int32_t {
        const int b = call_base_num(base);
        if (b < 0) { *wrong = 1; return 0; }
        return call_cell(S, FLANK, b, 3) + call_cell(S, FLANK, b + 4, 3) + call_cell(S, FLANK, b, 0) + call_cell(S, FLANK, b + 4, 0);
    };
    int wrong = 0;
    int32_t supported = 0;
    const int32_t ins = call_sum(S, FLANK + 1, 1), del = call_sum(S, FLANK + 1, 2), snps = call_sum(S, FLANK + 1, 3);
    if (is_ref) {
        const int b = call_base_num(REF[0]);
        supported = call_cell(S, FLANK, b, 0) + call_cell(S, FLANK, b + 4, 0);
    } else if (flags & ((1 << L_HOMO_SNP) | (1 << L_HET_SNP))) {
        supported = snp(ALT1[0], &wrong) + (multi ? snp(ALT2[0], &wrong) : 0);
    } else if (flags & ((1 << L_HOMO_INS) | (1 << L_INS_INS))) {
        supported = ins - snps;
    } else if (flags & (1 << L_ACGT_INS)) {
        supported = ins - snps + (multi ? snp(ALT1[0], &wrong) : 0);
    } else if (flags & ((1 << L_HOMO_DEL) | (1 << L_DEL_DEL))) {
        supported = del;
    } else if (flags & (1 << L_ACGT_DEL)) {
        supported = del + (multi ? snp(ALT2[0], &wrong) : 0);
    } else {
        supported = ins + del - snps;
    }
    // gt21_enum_from and genotype_enum_for_task
    int gt21;
    if (multi) gt21 = call_mix(call_partial(ref_len, ALT1, alt1_len), call_partial(ref_len, ALT2, alt2_len));
    else if (genotype == 1) gt21 = call_mix(call_partial(ref_len, ALT1, alt1_len), call_partial(ref_len, ALT1, alt1_len));
    else gt21 = call_mix(call_partial(ref_len, REF, ref_len), call_partial(ref_len, ALT1, alt1_len));
    if (gt21 < 0 || wrong) return MPN_CALL_RAISES;
    const int task = genotype == 3 ? 2 : genotype;
    row->site = 0; row->flags = flags; row->genotype = genotype; row->gt21 = gt21; row->genotype_task = task;
    row->p = call_mul(gt[gt21], g[task]);
    row->supported = supported; row->depth = depth;
    row->ref_len = ref_len; row->alt1_len = alt1_len; row->alt2_len = alt2_len; row->reserved = 0;
    return MPN_CALL_EMITTED;
}

// float32(rint(double(p) * 1e6) / 1e6): p * 1e6 is exact in float64 (24 bits times 15625 * 2^6), so rint rounds what %.6f rounds
CALL_HD float call_quantize(float p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__ddiv_rn(rint((double)p * 1.0e6), 1.0e6);
#else
    return (float)(__builtin_rint((double)p * 1.0e6) / 1.0e6);
#endif
}

}  // namespace mpn_call
