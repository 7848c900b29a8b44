// What the device BAM writer (csrc/bam_out_kernels.hip, include/mpn_bam.h) decides, in one place for the device and the host: the
// field rules of a SAM line, the size of its BAM record, the float rule of `f` tags, reg2bin, the BGZF block cut and the BAI
// builder.  Like name_set_core.h and pileup_core.h it compiles for the device and, with plain g++, for the host:
// scripts/bam_out_host_check.cpp runs scan, encode, cut and bai_build serially through it under the host's sanitizers.
//
// The rule of the whole path: a record is written exactly as bam.encode_record / mpn_bam_encode write it, or it is refused with one
// of the MPN_SAM_* statuses of mpn_bam.h; nothing is guessed.  A line with several faults reports the one with the smallest code
// (bo_worse), so that the order in which a wave or a serial loop meets them does not matter.
//
// Record layout (SAMv1 4.2, without the block_size word): 32 fixed bytes | QNAME + NUL | n_cigar x u32 | (l_seq + 1) / 2 packed
// bases | l_seq qualities | aux fields [| CG:B,I + the real CIGAR when it has more than 65535 operations].
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/mpn_bam.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BO_HD __host__ __device__ __forceinline__
#else
#define BO_HD inline
#endif

namespace mpn {
namespace bo {

constexpr int32_t BO_MAX_CIGAR_OPS = 65535;          // n_cigar_op is 16 bits wide
constexpr int64_t BO_MAX_OP_LEN = (1 << 28) - 1;     // an operation's length has 28 bits
constexpr int64_t BO_BLOCK = 0xff00;                 // payload bytes of a BGZF block (bam.BGZF_BLOCK)
constexpr int64_t BO_MAX_END = (int64_t)1 << 29;     // the end of the binning scheme: 512 Mbp
constexpr int64_t BO_SAT = 100000000000000000LL;     // 10^17: where bo_parse_int stops counting (ten times it still fits)

// what the scan leaves per line for the encode, the sort, the cut and the index (all 32-bit: a line is shorter than 2^31 bytes)
struct BoRec {
    int32_t tid, pos0, end0, flag, mapq, ntid, pnext0, tlen;
    int32_t n_ops;        // operations of the CIGAR text (the record holds 2 when there are more than BO_MAX_CIGAR_OPS)
    int32_t l_seq, ref_len, aux_size;
    int32_t size;         // bytes of the record; 0 unless status is MPN_SAM_OK
    int32_t status;
    int32_t pad[2];
};
static_assert(sizeof(BoRec) == 64, "one record summary is 64 bytes");

BO_HD int32_t bo_worse(int32_t a, int32_t b) { return a == 0 ? b : (b == 0 ? a : (a < b ? a : b)); }
BO_HD bool bo_refused(int32_t status) { return status >= MPN_SAM_FEW_FIELDS; }
BO_HD bool bo_is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }   // what bytes.strip() strips
BO_HD bool bo_is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

BO_HD int reg2bin(int64_t beg, int64_t end) {
    --end;
    int s = 14, t = ((1 << 15) - 1) / 7;
    for (int l = 5; l > 0; --l) {
        if (beg >> s == end >> s) return t + (int)(beg >> s);
        s += 3;
        t -= 1 << (3 * (l - 1));
    }
    return 0;
}

// p[a .. b) as -?[0-9]+ -> 0 and *v (stopping at +-BO_SAT: every range that is asked about lies far inside), or MPN_SAM_NOT_NUMBER
BO_HD int32_t bo_parse_int(const uint8_t *p, int32_t a, int32_t b, int64_t *v) {
    const bool neg = a < b && p[a] == '-';
    if (neg) ++a;
    if (a >= b) return MPN_SAM_NOT_NUMBER;
    int64_t x = 0;
    for (int32_t i = a; i < b; ++i) {
        if (!bo_is_digit(p[i])) return MPN_SAM_NOT_NUMBER;
        if (x < BO_SAT) x = x * 10 + (p[i] - '0');
    }
    *v = neg ? -x : x;
    return 0;
}

BO_HD int bo_cigar_op(uint8_t c) {
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; default: return -1;
    }
}
BO_HD bool bo_ref_consuming(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// the operation whose letter is p[at], with its digits p[from .. at): 0 and the word's halves, or a status
BO_HD int32_t bo_cigar_one(const uint8_t *p, int32_t from, int32_t at, int *op, int64_t *num) {
    *op = bo_cigar_op(p[at]);
    if (*op < 0) return MPN_SAM_CIGAR_OP;
    if (from >= at) return MPN_SAM_CIGAR_NUM;
    int64_t x = 0;
    for (int32_t i = from; i < at; ++i)
        if (x <= BO_MAX_OP_LEN) x = x * 10 + (p[i] - '0');
    if (x > BO_MAX_OP_LEN) return MPN_SAM_CIGAR_NUM;
    *num = x;
    return 0;
}

BO_HD uint8_t bo_seq_code(uint8_t c) {       // bam._SEQ_TABLE: the letters of =ACMGRSVTWYHKDBN in either case, 15 for the rest
    if (c >= 'a' && c <= 'z') c -= 32;
    switch (c) {
        case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5;
        case 'S': return 6; case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11;
        case 'K': return 12; case 'D': return 13; case 'B': return 14; default: return 15;
    }
}

// The float rule.  p[a .. b) of the forms -?digits and -?digits.digits, with at most 15 significant digits and at most 22 digits
// behind the point: m (all digits as one integer, below 2^53) and 10^d are exact doubles, one IEEE division rounds their quotient
// correctly, and that is the double strtod returns; the conversion to float is the one `(float)strtod(text)` makes.
BO_HD int32_t bo_parse_float(const uint8_t *p, int32_t a, int32_t b, uint32_t *bits) {
    const bool neg = a < b && p[a] == '-';
    if (neg) ++a;
    int64_t m = 0;
    int32_t sig = 0, d = 0, n_int = 0;
    bool point = false;
    for (int32_t i = a; i < b; ++i) {
        const uint8_t c = p[i];
        if (c == '.') {
            if (point || n_int == 0) return MPN_SAM_TAG_FLOAT;
            point = true;
        } else if (bo_is_digit(c)) {
            if (point) ++d; else ++n_int;
            if (sig > 0 || c != '0') ++sig;
            if (sig > 15 || d > 22) return MPN_SAM_TAG_FLOAT;
            m = m * 10 + (c - '0');
        } else return MPN_SAM_TAG_FLOAT;
    }
    if (n_int == 0 || (point && d == 0)) return MPN_SAM_TAG_FLOAT;
    double den = 1.0;
    for (int32_t k = 0; k < d; ++k) den *= 10.0;      // (exact: every power of ten up to 10^22 is a double)
    const double q = (double)m / den;
    const float f = (float)(neg ? -q : q);
    memcpy(bits, &f, 4);
    return 0;
}

// ---- aux fields ----------------------------------------------------------------------------------------------------------------------
struct BoAux {
    int32_t size;        // bytes in the record
    uint32_t value;      // A: the character; i: the integer's low 32 bits; f: the float's bits
    uint8_t code;        // the type byte that is written: A c C s S i I f Z H
    uint8_t width;       // bytes of `value` that are written (Z / H: 0, the text follows)
};

// the field p[a .. b) -> 0 and what it becomes, or a status
BO_HD int32_t bo_aux_head(const uint8_t *p, int32_t a, int32_t b, BoAux *x) {
    x->size = 0; x->value = 0; x->code = 0; x->width = 0;
    if (b - a < 5 || p[a + 2] != ':' || p[a + 4] != ':') return MPN_SAM_TAG_FORM;
    const uint8_t typ = p[a + 3];
    const int32_t v0 = a + 5;
    if (typ == 'A') {
        if (v0 >= b) return MPN_SAM_TAG_FORM;       // (an empty value: the two existing encoders disagree about it)
        x->code = 'A'; x->value = p[v0]; x->width = 1;
    } else if (typ == 'i') {
        int64_t v;
        if (bo_parse_int(p, v0, b, &v)) return MPN_SAM_TAG_INT;
        if (v >= 0) {
            if (v <= 0xff) { x->code = 'C'; x->width = 1; }
            else if (v <= 0xffff) { x->code = 'S'; x->width = 2; }
            else if (v <= 0xffffffffLL) { x->code = 'I'; x->width = 4; }
            else return MPN_SAM_TAG_INT;
        } else {
            if (v >= -0x80) { x->code = 'c'; x->width = 1; }
            else if (v >= -0x8000) { x->code = 's'; x->width = 2; }
            else if (v >= -0x80000000LL) { x->code = 'i'; x->width = 4; }
            else return MPN_SAM_TAG_INT;
        }
        x->value = (uint32_t)(uint64_t)v;
    } else if (typ == 'f') {
        if (bo_parse_float(p, v0, b, &x->value)) return MPN_SAM_TAG_FLOAT;
        x->code = 'f'; x->width = 4;
    } else if (typ == 'Z' || typ == 'H') {
        x->code = typ;
        x->size = 3 + (b - v0) + 1;
        return 0;
    } else if (typ == 'B') return MPN_SAM_TAG_ARRAY;
    else return MPN_SAM_TAG_TYPE;
    x->size = 3 + x->width;
    return 0;
}

// everything of the field but the text of a Z / H value (out[3 .. size - 1) there; the NUL is written here)
BO_HD void bo_aux_put(const uint8_t *p, int32_t a, const BoAux &x, uint8_t *out) {
    out[0] = p[a]; out[1] = p[a + 1]; out[2] = x.code;
    for (int k = 0; k < x.width; ++k) out[3 + k] = (uint8_t)(x.value >> (8 * k));
    if (x.width == 0) out[x.size - 1] = 0;
}

BO_HD void bo_put32(uint8_t *out, uint32_t v) {
    out[0] = (uint8_t)v; out[1] = (uint8_t)(v >> 8); out[2] = (uint8_t)(v >> 16); out[3] = (uint8_t)(v >> 24);
}

// ---- the numeric fields, the sizes and the fixed part -------------------------------------------------------------------------------
// tab[k]: where field k ends (k = 0..10; tab[10] is the eleventh tab or the end of the line); field k starts behind tab[k - 1]
BO_HD int32_t bo_field_start(const int32_t *tab, int k) { return k == 0 ? 0 : tab[k - 1] + 1; }

// FLAG POS MAPQ PNEXT TLEN (which = 0..4) into r -> 0 or a status.  POS is 0 .. 2^31 - 1: the sort key takes no negative one.
BO_HD int32_t bo_numeric_field(const uint8_t *p, const int32_t *tab, int which, BoRec *r) {
    const int k = which == 0 ? 1 : which == 1 ? 3 : which == 2 ? 4 : which == 3 ? 7 : 8;
    int64_t v;
    if (bo_parse_int(p, bo_field_start(tab, k), tab[k], &v)) return MPN_SAM_NOT_NUMBER;
    switch (which) {
        case 0: if (v < 0 || v > 65535) return MPN_SAM_NUM_RANGE; r->flag = (int32_t)v; break;
        case 1: if (v < 0 || v > 0x7fffffffLL) return MPN_SAM_NUM_RANGE; r->pos0 = (int32_t)(v - 1); break;
        case 2: if (v < 0 || v > 255) return MPN_SAM_NUM_RANGE; r->mapq = (int32_t)v; break;
        case 3: if (v - 1 < -0x80000000LL || v - 1 > 0x7fffffffLL) return MPN_SAM_NUM_RANGE; r->pnext0 = (int32_t)(v - 1); break;
        default: if (v < -0x80000000LL || v > 0x7fffffffLL) return MPN_SAM_NUM_RANGE; r->tlen = (int32_t)v; break;
    }
    return 0;
}

// after tid, flag, pos0, n_ops, l_seq, aux_size and the CIGAR's reference length are known: end0, the size, the last refusals
BO_HD int32_t bo_finish_rec(const int32_t *tab, int64_t ref_len, BoRec *r) {
    int32_t st = 0;
    const int32_t l_name = tab[0] + 1;
    if (l_name > 255) st = bo_worse(st, MPN_SAM_QNAME_LONG);
    const int64_t end0 = (ref_len > 0 && !(r->flag & 4)) ? (int64_t)r->pos0 + ref_len : (int64_t)r->pos0 + 1;
    if (end0 > BO_MAX_END) st = bo_worse(st, MPN_SAM_NUM_RANGE);      // (behind it reg2bin does not fit the record's 16 bits)
    int64_t size = 32 + (int64_t)l_name + (r->l_seq + 1) / 2 + (int64_t)r->l_seq + r->aux_size;
    if (r->n_ops > BO_MAX_CIGAR_OPS) {
        // <l_seq>S<ref_len>N: both lengths have to fit an operation
        if (ref_len > BO_MAX_OP_LEN || r->l_seq > BO_MAX_OP_LEN) st = bo_worse(st, MPN_SAM_CIGAR_NUM);
        size += 8 + 8 + 4 * (int64_t)r->n_ops;
    } else size += 4 * (int64_t)r->n_ops;
    if (size > 0x7fffffffLL) st = bo_worse(st, MPN_SAM_NUM_RANGE);
    r->end0 = (int32_t)end0;
    r->ref_len = (int32_t)(ref_len > 0x7fffffffLL ? 0x7fffffffLL : ref_len);
    r->size = (int32_t)size;
    return st;
}

BO_HD void bo_put_fixed(const BoRec &r, int32_t l_name, uint8_t *out) {
    const int32_t n_cigar = r.n_ops > BO_MAX_CIGAR_OPS ? 2 : r.n_ops;
    bo_put32(out, (uint32_t)r.tid);
    bo_put32(out + 4, (uint32_t)r.pos0);
    out[8] = (uint8_t)l_name; out[9] = (uint8_t)r.mapq;
    const int bin = reg2bin(r.pos0, r.end0);
    out[10] = (uint8_t)bin; out[11] = (uint8_t)(bin >> 8);
    out[12] = (uint8_t)n_cigar; out[13] = (uint8_t)(n_cigar >> 8);
    out[14] = (uint8_t)r.flag; out[15] = (uint8_t)(r.flag >> 8);
    bo_put32(out + 16, (uint32_t)r.l_seq);
    bo_put32(out + 20, (uint32_t)r.ntid);
    bo_put32(out + 24, (uint32_t)r.pnext0);
    bo_put32(out + 28, (uint32_t)r.tlen);
}

// ---- the serial form of scan and encode (the host check; the kernels do the same work a wave per line) -------------------------------
// lookup(p, len) -> index of the reference with these bytes or -1
template <class Lookup>
inline void bo_scan_line(const uint8_t *p, int32_t len, int32_t exclude_flags, const Lookup &lookup, int32_t *tab, BoRec *r) {
    memset(r, 0, sizeof(*r));
    if (len > 0 && p[len - 1] == '\n') --len;
    int32_t n_tab = 0;
    bool cr = false, text = false;
    for (int32_t i = 0; i < len; ++i) {
        if (p[i] == '\t') { if (n_tab < 11) tab[n_tab] = i; ++n_tab; }
        cr |= p[i] == '\r';
        text |= !bo_is_space(p[i]);
    }
    if ((len > 0 && p[0] == '@') || !text) { r->status = MPN_SAM_SKIPPED; r->flag = text; return; }      // flag 1: a header line
    if (cr) { r->status = MPN_SAM_CR; return; }
    if (n_tab < 10) { r->status = MPN_SAM_FEW_FIELDS; return; }
    if (n_tab == 10) tab[10] = len;
    int32_t st = bo_numeric_field(p, tab, 0, r);
    if (st) { r->status = st; return; }
    if (r->flag & exclude_flags) { r->status = MPN_SAM_EXCLUDED; return; }
    for (int w = 1; w < 5; ++w) st = bo_worse(st, bo_numeric_field(p, tab, w, r));
    auto ref_of = [&](int k) -> int32_t {
        const int32_t a = bo_field_start(tab, k), n = tab[k] - a;
        return (n == 1 && p[a] == '*') ? -1 : lookup(p + a, n);
    };
    r->tid = ref_of(2);
    r->ntid = (tab[6] - bo_field_start(tab, 6) == 1 && p[bo_field_start(tab, 6)] == '=') ? r->tid : ref_of(6);
    // CIGAR
    int64_t ref_len = 0;
    {
        const int32_t a = bo_field_start(tab, 5), b = tab[5];
        if (!(b - a == 1 && p[a] == '*')) {
            int32_t from = a;
            for (int32_t i = a; i < b; ++i)
                if (!bo_is_digit(p[i])) {
                    int op;
                    int64_t num;
                    const int32_t s1 = bo_cigar_one(p, from, i, &op, &num);
                    st = bo_worse(st, s1);
                    if (!s1 && bo_ref_consuming(op)) ref_len += num;
                    ++r->n_ops;
                    from = i + 1;
                }
            if (from != b) st = bo_worse(st, MPN_SAM_CIGAR_NUM);      // digits without an operation behind them
        }
    }
    {
        const int32_t a = bo_field_start(tab, 9), n = tab[9] - a;
        r->l_seq = (n == 1 && p[a] == '*') ? 0 : n;
        const int32_t qa = bo_field_start(tab, 10), qn = tab[10] - qa;
        if (r->l_seq > 0 && !(qn == 1 && p[qa] == '*') && qn != r->l_seq) st = bo_worse(st, MPN_SAM_QUAL_LEN);
    }
    int64_t aux = 0;
    for (int32_t a = tab[10]; a < len;) {           // a: a tab in front of an aux field
        int32_t b = a + 1;
        while (b < len && p[b] != '\t') ++b;
        BoAux x;
        st = bo_worse(st, bo_aux_head(p, a + 1, b, &x));
        aux += x.size;
        a = b;
    }
    if (aux > 0x7fffffffLL) { st = bo_worse(st, MPN_SAM_NUM_RANGE); aux = 0; }
    r->aux_size = (int32_t)aux;
    st = bo_worse(st, bo_finish_rec(tab, ref_len, r));
    r->status = st;
    if (st) r->size = 0;
}

// the record of a line whose scan said MPN_SAM_OK, into out[0 .. r.size)
inline void bo_encode_line(const uint8_t *p, int32_t len, const int32_t *tab, const BoRec &r, uint8_t *out) {
    if (len > 0 && p[len - 1] == '\n') --len;
    const int32_t l_name = tab[0] + 1;
    bo_put_fixed(r, l_name, out);
    uint8_t *o = out + 32;
    memcpy(o, p, (size_t)tab[0]);
    o[tab[0]] = 0;
    o += l_name;
    const bool long_cigar = r.n_ops > BO_MAX_CIGAR_OPS;
    uint8_t *cg = out + r.size - 4 * (int64_t)r.n_ops;      // where the real CIGAR goes when it is long
    if (long_cigar) {
        bo_put32(o, (uint32_t)r.l_seq << 4 | 4u);
        bo_put32(o + 4, (uint32_t)r.ref_len << 4 | 3u);
        memcpy(cg - 8, "CGBI", 4);
        bo_put32(cg - 4, (uint32_t)r.n_ops);
    }
    {
        const int32_t a = bo_field_start(tab, 5), b = tab[5];
        int32_t from = a, k = 0;
        if (!(b - a == 1 && p[a] == '*'))
            for (int32_t i = a; i < b; ++i)
                if (!bo_is_digit(p[i])) {
                    int op;
                    int64_t num;
                    bo_cigar_one(p, from, i, &op, &num);
                    bo_put32((long_cigar ? cg : o) + 4 * (int64_t)k, (uint32_t)num << 4 | (uint32_t)op);
                    ++k;
                    from = i + 1;
                }
    }
    o += long_cigar ? 8 : 4 * (int64_t)r.n_ops;
    const uint8_t *sq = p + bo_field_start(tab, 9);
    for (int32_t j = 0; j < (r.l_seq + 1) / 2; ++j)
        o[j] = (uint8_t)(bo_seq_code(sq[2 * j]) << 4 | (2 * j + 1 < r.l_seq ? bo_seq_code(sq[2 * j + 1]) : 0));
    o += (r.l_seq + 1) / 2;
    const int32_t qa = bo_field_start(tab, 10);
    const bool no_qual = tab[10] - qa == 1 && p[qa] == '*';
    for (int32_t j = 0; j < r.l_seq; ++j) o[j] = no_qual ? 0xff : (uint8_t)(p[qa + j] - 33);
    o += r.l_seq;
    for (int32_t a = tab[10]; a < len;) {
        int32_t b = a + 1;
        while (b < len && p[b] != '\t') ++b;
        BoAux x;
        bo_aux_head(p, a + 1, b, &x);
        bo_aux_put(p, a + 1, x, o);
        if (x.width == 0) memcpy(o + 3, p + a + 6, (size_t)(x.size - 4));
        o += x.size;
        a = b;
    }
}

}  // namespace bo
}  // namespace mpn

// ---- host code: the block cut and the index ------------------------------------------------------------------------------------------
#include <algorithm>
#include <map>
#include <vector>

namespace mpn {
namespace bo {

// BgzfWriter.write / flush / flush_try over the payload STREAM: the BAM header, then per record its block_size word and its bytes.
// The blocks are a partition of that stream, so a cut is the ascending list of the stream offsets at which blocks start.  A virtual
// offset is provisional here (block NUMBER << 16 | offset in the block), as BgzfWriter.tell() has it.
struct BoCut {
    std::vector<int64_t> block_start;     // n_blocks + 1 entries once closed: block i is stream[block_start[i] .. block_start[i + 1])
    int64_t pos = 0;                      // bytes of the stream so far
    BoCut() { block_start.push_back(0); }
    int64_t fill() const { return pos - block_start.back(); }
    void flush() { if (fill() > 0) block_start.push_back(pos); }
    void write(int64_t bytes) {
        pos += bytes;
        while (fill() >= BO_BLOCK) block_start.push_back(block_start.back() + BO_BLOCK);
    }
    uint64_t tell() const { return (uint64_t)(block_start.size() - 1) << 16 | (uint64_t)fill(); }
    // the BAM header: its blocks are closed before the first record -> the virtual offset of the first record
    uint64_t header(int64_t bytes) { write(bytes); flush(); return tell(); }
    // a record of rec_size bytes (without its block_size word) -> the virtual offset behind it
    uint64_t record(int64_t rec_size) {
        if (fill() + 4 + rec_size > BO_BLOCK) flush();
        write(4 + rec_size);
        return tell();
    }
    // the last block is closed -> the virtual offset of the end of the data (where the EOF block starts)
    uint64_t close() { flush(); return tell(); }
    int64_t n_blocks() const { return (int64_t)block_start.size() - 1; }
};

// provisional -> real virtual offset; addr[i]: the file address of block i (n_blocks + 1 entries)
inline uint64_t bo_resolve(uint64_t voff, const int64_t *addr) { return (uint64_t)addr[voff >> 16] << 16 | (voff & 0xffff); }

// bam.BaiBuilder (htslib's hts_idx_push / hts_idx_finish for min_shift 14, 5 levels) over records in file order, with REAL virtual
// offsets: push for every record, finish, linear, write.  -> the bytes of the .bai file
inline std::vector<uint8_t> bai_build(int32_t n_ref, int64_t n, const int32_t *tid, const int32_t *pos0, const int32_t *end0, const uint64_t *voff_after,
                                      const uint8_t *mapped, uint64_t voff_first, uint64_t voff_end) {
    constexpr uint32_t NONE = 0xffffffffu, META = 37450;
    constexpr uint64_t NO_OFF = ~(uint64_t)0;
    struct Chunk { uint64_t beg, end; };
    std::vector<std::map<uint32_t, std::vector<Chunk>>> bins((size_t)n_ref);
    std::vector<std::vector<uint64_t>> lin((size_t)n_ref);
    uint64_t n_no_coor = 0, last_off = voff_first, save_off = voff_first, off_beg = voff_first, n_mapped = 0, n_unmapped = 0;
    uint32_t last_bin = NONE, save_bin = NONE;
    int32_t last_tid = -1, save_tid = -1;
    bool first = true;
    auto chunk = [&](int32_t t, uint32_t b, uint64_t beg, uint64_t end) {
        if (t < 0) t += n_ref;                     // (Python's bins[-1]; never reached on sorted input)
        if (t >= 0 && t < n_ref) bins[(size_t)t][b].push_back(Chunk{beg, end});
    };
    for (int64_t i = 0; i < n; ++i) {
        const int32_t t = tid[i];
        int64_t beg = pos0[i], end = end0[i];
        if (t < 0) { beg = -1; end = 0; }
        if (last_tid != t || first) { last_tid = t; last_bin = NONE; first = false; }
        if (t >= 0) {
            if (mapped[i] && t < n_ref) {
                const int64_t b0 = std::max<int64_t>(beg, 0), e0 = end > 0 ? end : 1;
                std::vector<uint64_t> &l = lin[(size_t)t];
                const int64_t w1 = ((e0 - 1) >> 14) + 1;
                if ((int64_t)l.size() < w1) l.resize((size_t)w1, NO_OFF);
                for (int64_t w = b0 >> 14; w < w1; ++w) if (l[(size_t)w] == NO_OFF) l[(size_t)w] = last_off;
            }
        } else ++n_no_coor;
        const uint32_t b = (uint32_t)reg2bin(beg, end);
        if (last_bin != b) {
            if (save_bin != NONE) chunk(save_tid, save_bin, save_off, last_off);
            if (last_bin == NONE && save_bin != NONE) {       // change of reference: close its pseudo-bin
                chunk(save_tid, META, off_beg, last_off);
                chunk(save_tid, META, n_mapped, n_unmapped);
                n_mapped = n_unmapped = 0;
                off_beg = last_off;
            }
            save_off = last_off;
            save_bin = last_bin = b;
            save_tid = t;
        }
        if (mapped[i]) ++n_mapped; else ++n_unmapped;
        last_off = voff_after[i];
    }
    if (save_tid >= 0) {
        chunk(save_tid, save_bin, save_off, voff_end);
        chunk(save_tid, META, off_beg, voff_end);
        chunk(save_tid, META, n_mapped, n_unmapped);
    }
    const uint32_t n_bins = META - 1;
    auto by_beg = [](const Chunk &a, const Chunk &b) { return a.beg < b.beg; };
    for (auto &bm : bins) {
        // bins whose chunks span less than 64 KiB of the file are folded into their parents, bottom level first
        for (int lvl = 5; lvl > 0; --lvl) {
            const uint32_t start = (uint32_t)(((1u << (3 * lvl)) - 1) / 7);
            std::vector<uint32_t> keys;
            for (const auto &kv : bm) if (kv.first >= start && kv.first < n_bins) keys.push_back(kv.first);
            for (uint32_t b : keys) {
                std::vector<Chunk> &lst = bm[b];
                if (lvl < 5 && lst.size() > 1) std::stable_sort(lst.begin(), lst.end(), by_beg);
                const uint32_t parent = (b - 1) >> 3;
                if ((int64_t)(lst.back().end >> 16) - (int64_t)(lst.front().beg >> 16) < 0x10000 && bm.count(parent)) {
                    std::vector<Chunk> &pl = bm[parent];
                    pl.insert(pl.end(), lst.begin(), lst.end());
                    bm.erase(b);
                }
            }
        }
        if (bm.count(0)) std::stable_sort(bm[0].begin(), bm[0].end(), by_beg);
        for (auto &kv : bm) {
            if (kv.first >= n_bins) continue;
            std::vector<Chunk> merged{kv.second[0]};
            for (size_t k = 1; k < kv.second.size(); ++k) {
                const Chunk c = kv.second[k];
                if (merged.back().end >> 16 >= c.beg >> 16) merged.back().end = std::max(merged.back().end, c.end);
                else merged.push_back(c);
            }
            kv.second.swap(merged);
        }
    }
    std::vector<uint8_t> out;
    auto put = [&](const void *v, size_t k) { const uint8_t *q = (const uint8_t *)v; out.insert(out.end(), q, q + k); };
    put("BAI\1", 4);
    put(&n_ref, 4);
    for (int32_t t = 0; t < n_ref; ++t) {
        const int32_t nb = (int32_t)bins[(size_t)t].size();
        put(&nb, 4);
        for (const auto &kv : bins[(size_t)t]) {
            const int32_t nc = (int32_t)kv.second.size();
            put(&kv.first, 4);
            put(&nc, 4);
            for (const Chunk &c : kv.second) { put(&c.beg, 8); put(&c.end, 8); }
        }
        std::vector<uint64_t> l = lin[(size_t)t];
        for (int64_t w = (int64_t)l.size() - 2; w >= 0; --w) if (l[(size_t)w] == NO_OFF) l[(size_t)w] = l[(size_t)w + 1];
        for (uint64_t &x : l) if (x == NO_OFF) x = 0;
        const int32_t nl = (int32_t)l.size();
        put(&nl, 4);
        if (nl) put(l.data(), (size_t)nl * 8);
    }
    put(&n_no_coor, 8);
    return out;
}

}  // namespace bo
}  // namespace mpn
