// The serial gzip decoder behind mpn_gzip_inflate (include/mpn_ingest.h), written from RFC 1951 and RFC 1952.  It compiles for
// the device (one lane of csrc/inflate_kernels.hip runs it) and for the host (scripts/inflate_host_check.cpp runs every test case
// through it under the sanitizers): tables and window come in as pointers, nothing here knows about LDS.
//
// inf_run() decodes until the 32 KiB window ring holds INF_HALF bytes that have not been flushed, until a member's deflate stream
// has ended, or until the stream is finished (status set).  The caller then flushes ring[flushed .. out_pos) -- stores what the
// slot can take, folds the bytes into the member's CRC-32 -- and calls again.  After the flush that follows a member's last block
// the next call checks the trailer against that CRC (the CRC arithmetic is in crc32_poly.h).  Bounds: every read of the input is
// checked against in_end, every ring index is masked, and each pass of the symbol loop consumes at least one bit or leaves.
#pragma once
#include <stdint.h>
#include "../../include/mpn_ingest.h"
#include "crc32_poly.h"

#if defined(__HIPCC__)
#define INF_HD __host__ __device__ inline
#else
#define INF_HD inline
#endif

namespace mpn_inf {

constexpr int INF_WIN = 32768, INF_MASK = INF_WIN - 1;
constexpr int INF_HALF = 16384;          // a flush is due when this much is pending; a match adds at most 257 more
constexpr int INF_FAST_BITS = 10;
constexpr int INF_MAX_LENS = 320;        // 288 + 32

// A canonical code: symbols ordered by (length, symbol) with the count per length (decoded bit by bit, as RFC 1951 3.2.2 orders
// them), and a table over the next INF_FAST_BITS bits for the codes that short: symbol << 4 | length, 0 = look further.
struct InfCode {
    uint16_t count[16];
    uint16_t sym[288];
    uint16_t fast[1 << INF_FAST_BITS];
};

enum { INF_PH_HEADER = 0, INF_PH_BLOCK, INF_PH_STORED, INF_PH_SYMS, INF_PH_TRAILER, INF_PH_DONE };
enum { INF_CODES = 0, INF_LENS = 1, INF_DISTS = 2 };

struct InfState {
    int64_t ip, in_end;       // next input byte, end of the stream (offsets into the pointer inf_run gets)
    uint64_t buf;             // bit buffer, the next bit is bit 0
    int nb;                   // bits in buf
    int64_t out_pos;          // bytes produced by the stream so far, all members
    int64_t member_start;     // out_pos where the current member began: distances must not reach before it
    int64_t flushed;          // bytes the caller has flushed
    uint32_t crc;             // CRC register of the current member over the flushed bytes (starts as all ones)
    uint32_t stored_left;
    int phase, last, members, status;
};

INF_HD void inf_init(InfState *s, int64_t in_begin, int64_t in_end) {
    s->ip = in_begin; s->in_end = in_end; s->buf = 0; s->nb = 0;
    s->out_pos = 0; s->member_start = 0; s->flushed = 0; s->crc = 0xFFFFFFFFu; s->stored_left = 0;
    s->phase = INF_PH_HEADER; s->last = 0; s->members = 0; s->status = MPN_INFLATE_OK;
}

// ---- codes ----
// lens[0..n) -> code.  0 or MPN_INFLATE_BAD_CODE.  As zlib: an over-subscribed code is refused; an incomplete one is refused too,
// except a literal/length or distance code that is ONE code of one bit (RFC 1951 3.2.7) and a distance code without any code.
INF_HD int inf_build(InfCode *c, const uint8_t *lens, int n, int kind) {
    uint16_t offs[16];
    for (int l = 0; l < 16; ++l) c->count[l] = 0;
    for (int i = 0; i < n; ++i) c->count[lens[i] & 15]++;
    const int used = n - c->count[0];
    c->count[0] = 0;
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - c->count[l];
        if (left < 0) return MPN_INFLATE_BAD_CODE;
    }
    if (left > 0) {
        const bool one_bit = used == 1 && c->count[1] == 1;
        if (kind == INF_CODES || !(one_bit || (used == 0 && kind == INF_DISTS))) return MPN_INFLATE_BAD_CODE;
    }
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + c->count[l]);
    for (int i = 0; i < n; ++i) if (lens[i] & 15) c->sym[offs[lens[i] & 15]++] = (uint16_t)i;
    for (int j = 0; j < (1 << INF_FAST_BITS); ++j) c->fast[j] = 0;
    uint32_t code = 0;
    int idx = 0;
    for (int l = 1; l <= INF_FAST_BITS; ++l) {
        for (int k = 0; k < (int)c->count[l]; ++k, ++idx, ++code) {
            uint32_t rev = 0;
            for (int b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
            const uint16_t e = (uint16_t)(c->sym[idx] << 4 | l);
            for (uint32_t j = rev; j < (1u << INF_FAST_BITS); j += 1u << l) c->fast[j] = e;
        }
        code <<= 1;
    }
    return 0;
}

// The symbol the next bits spell, *len = its length.  -1: no symbol (incomplete code); -2: the input ends inside the code.
INF_HD int inf_decode(const InfCode *c, uint64_t bits, int avail, int *len) {
    const uint16_t e = c->fast[bits & ((1u << INF_FAST_BITS) - 1)];
    if (e) {
        *len = e & 15;
        return (e & 15) > avail ? -2 : e >> 4;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        if (l > avail) return -2;
        code |= (int)((bits >> (l - 1)) & 1);
        const int cnt = c->count[l];
        if (code - cnt < first) { *len = l; return c->sym[index + (code - first)]; }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

INF_HD void inf_refill(InfState *s, const uint8_t *in) {
    if (s->ip + 8 <= s->in_end) {
        uint64_t w;
        __builtin_memcpy(&w, in + s->ip, 8);
        s->buf |= s->nb < 64 ? w << s->nb : 0;
        const int adv = (63 - s->nb) >> 3;
        s->ip += adv;
        s->nb += adv * 8;
        return;
    }
    while (s->nb <= 56 && s->ip < s->in_end) { s->buf |= (uint64_t)in[s->ip++] << s->nb; s->nb += 8; }
}
INF_HD void inf_drop(InfState *s, int n) { s->buf >>= n; s->nb -= n; }
// hand the whole bytes of the bit buffer back to the input; the bits of a started byte are dropped (RFC 1951 3.2.4, RFC 1952 2.3)
INF_HD void inf_to_bytes(InfState *s) {
    s->ip -= s->nb >> 3;
    s->buf = 0; s->nb = 0;
}

INF_HD int inf_fail(InfState *s, int status) { s->status = status; s->phase = INF_PH_DONE; return 1; }

// RFC 1952 2.3: the member header at ip.  Also decides what bytes after the last member are.
INF_HD void inf_header(InfState *s, const uint8_t *in) {
    const int64_t rem = s->in_end - s->ip;
    if (rem == 0) { s->phase = INF_PH_DONE; return; }
    if (!(rem >= 2 && in[s->ip] == 0x1f && in[s->ip + 1] == 0x8b)) {
        bool zeros = s->members > 0;
        for (int64_t k = s->ip; zeros && k < s->in_end; ++k) zeros = in[k] == 0;
        if (zeros) s->phase = INF_PH_DONE; else inf_fail(s, MPN_INFLATE_BAD_MAGIC);
        return;
    }
    if (rem < 10) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
    if (in[s->ip + 2] != 8) { inf_fail(s, MPN_INFLATE_BAD_MAGIC); return; }
    const int flg = in[s->ip + 3];
    int64_t p = s->ip + 10;
    if (flg & 4) {                                                     // FEXTRA
        if (s->in_end - p < 2) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
        const int64_t xlen = in[p] | in[p + 1] << 8;
        p += 2;
        if (s->in_end - p < xlen) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
        p += xlen;
    }
    for (int f = 8; f <= 16; f <<= 1) {                                // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        while (p < s->in_end && in[p]) ++p;
        if (p >= s->in_end) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
        ++p;
    }
    if (flg & 2) {                                                     // FHCRC
        if (s->in_end - p < 2) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
        p += 2;
    }
    s->ip = p;
    s->member_start = s->out_pos;
    s->crc = 0xFFFFFFFFu;
    s->phase = INF_PH_BLOCK;
}

// RFC 1952 2.3.1: CRC32 and ISIZE, against the register the flushes have kept
INF_HD void inf_trailer(InfState *s, const uint8_t *in) {
    if (s->in_end - s->ip < 8) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
    uint32_t v[2];
    for (int k = 0; k < 2; ++k) {
        const uint8_t *q = in + s->ip + 4 * k;
        v[k] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
    }
    if (v[0] != (s->crc ^ 0xFFFFFFFFu)) { inf_fail(s, MPN_INFLATE_BAD_CRC); return; }
    if (v[1] != (uint32_t)(s->out_pos - s->member_start)) { inf_fail(s, MPN_INFLATE_BAD_SIZE); return; }
    s->ip += 8;
    s->members++;
    s->phase = INF_PH_HEADER;
}

INF_HD void inf_end_block(InfState *s) {
    if (s->last) { inf_to_bytes(s); s->phase = INF_PH_TRAILER; }
    else s->phase = INF_PH_BLOCK;
}

// RFC 1951 3.2.3 - 3.2.7: the block header, and the codes of a compressed block.  lens: INF_MAX_LENS bytes of scratch.
INF_HD void inf_block(InfState *s, const uint8_t *in, InfCode *ll, InfCode *dc, uint8_t *lens) {
    inf_refill(s, in);
    if (s->nb < 3) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
    s->last = (int)(s->buf & 1);
    const int type = (int)((s->buf >> 1) & 3);
    inf_drop(s, 3);
    if (type == 3) { inf_fail(s, MPN_INFLATE_BAD_BLOCK); return; }
    if (type == 0) {
        inf_drop(s, s->nb & 7);
        inf_refill(s, in);
        if (s->nb < 32) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
        const uint32_t len = (uint32_t)(s->buf & 0xffff), nlen = (uint32_t)((s->buf >> 16) & 0xffff);
        inf_drop(s, 32);
        if ((len ^ nlen) != 0xffff) { inf_fail(s, MPN_INFLATE_BAD_BLOCK); return; }
        inf_to_bytes(s);
        s->stored_left = len;
        s->phase = INF_PH_STORED;
        return;
    }
    int hlit, hdist;
    if (type == 1) {
        hlit = 288; hdist = 32;       // (the symbols 286, 287, 30 and 31 have codes; meeting one is an error)
        for (int k = 0; k < 288; ++k) lens[k] = k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : 8;
        for (int k = 0; k < 32; ++k) lens[288 + k] = 5;
    } else {
        if (s->nb < 14) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
        hlit = (int)(s->buf & 31) + 257;
        hdist = (int)((s->buf >> 5) & 31) + 1;
        const int hclen = (int)((s->buf >> 10) & 15) + 4;
        inf_drop(s, 14);
        if (hlit > 286 || hdist > 30) { inf_fail(s, MPN_INFLATE_BAD_CODE); return; }
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (int k = 0; k < 19; ++k) lens[k] = 0;
        for (int k = 0; k < hclen; ++k) {
            inf_refill(s, in);
            if (s->nb < 3) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
            lens[order[k]] = (uint8_t)(s->buf & 7);
            inf_drop(s, 3);
        }
        if (inf_build(ll, lens, 19, INF_CODES)) { inf_fail(s, MPN_INFLATE_BAD_CODE); return; }
        int k = 0;
        while (k < hlit + hdist) {                    // every pass consumes a code of at least one bit
            inf_refill(s, in);
            int l = 0;
            const int sym = inf_decode(ll, s->buf, s->nb, &l);
            if (sym < 0) { inf_fail(s, sym == -2 ? MPN_INFLATE_TRUNCATED : MPN_INFLATE_BAD_CODE); return; }
            inf_drop(s, l);
            if (sym < 16) { lens[k++] = (uint8_t)sym; continue; }
            const int xb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
            if (s->nb < xb) { inf_fail(s, MPN_INFLATE_TRUNCATED); return; }
            const int rep = (sym == 16 ? 3 : sym == 17 ? 3 : 11) + (int)(s->buf & ((1u << xb) - 1));
            inf_drop(s, xb);
            if ((sym == 16 && k == 0) || k + rep > hlit + hdist) { inf_fail(s, MPN_INFLATE_BAD_CODE); return; }
            const uint8_t v = sym == 16 ? lens[k - 1] : 0;
            for (int j = 0; j < rep; ++j) lens[k++] = v;
        }
        if (lens[256] == 0) { inf_fail(s, MPN_INFLATE_BAD_CODE); return; }     // no way to end the block
    }
    // (building a code reads lens only: the literal/length code may overwrite the code-length code it was read with)
    if (inf_build(dc, lens + hlit, hdist, INF_DISTS) || inf_build(ll, lens, hlit, INF_LENS)) { inf_fail(s, MPN_INFLATE_BAD_CODE); return; }
    s->phase = INF_PH_SYMS;
}

// Decode on.  Returns 1 when the stream is finished (s->status), 0 when the caller has to flush and call again.
INF_HD int inf_run(InfState *s, const uint8_t *in, uint8_t *ring, InfCode *ll, InfCode *dc, uint8_t *lens) {
    for (;;) {      // every pass consumes input, produces output towards the next flush, or ends the stream
        switch (s->phase) {
        case INF_PH_DONE:
            return 1;
        case INF_PH_HEADER:
            inf_header(s, in);
            break;
        case INF_PH_TRAILER:
            if (s->flushed < s->out_pos) return 0;
            inf_trailer(s, in);
            break;
        case INF_PH_BLOCK:
            inf_block(s, in, ll, dc, lens);
            break;
        case INF_PH_STORED:
            while (s->stored_left) {
                if (s->out_pos - s->flushed >= INF_HALF) return 0;
                if (s->ip >= s->in_end) { inf_fail(s, MPN_INFLATE_TRUNCATED); break; }
                ring[s->out_pos & INF_MASK] = in[s->ip++];
                s->out_pos++;
                s->stored_left--;
            }
            if (s->phase == INF_PH_STORED) inf_end_block(s);
            break;
        case INF_PH_SYMS:
            for (;;) {
                if (s->out_pos - s->flushed >= INF_HALF) return 0;
                if (s->nb < 48) inf_refill(s, in);      // (a symbol takes 48 bits at most; a load per symbol is what the lane waits for)
                int l = 0;
                int sym = inf_decode(ll, s->buf, s->nb, &l);
                if (sym < 0) { inf_fail(s, sym == -2 ? MPN_INFLATE_TRUNCATED : MPN_INFLATE_BAD_CODE); break; }
                inf_drop(s, l);
                if (sym < 256) { ring[s->out_pos & INF_MASK] = (uint8_t)sym; s->out_pos++; continue; }
                if (sym == 256) { inf_end_block(s); break; }
                sym -= 257;
                if (sym >= 29) { inf_fail(s, MPN_INFLATE_BAD_CODE); break; }
                // RFC 1951 3.2.5.  With 48 bits or more at the top of the pass, 15 + 5 + 15 + 13 bits are there unless the input ends.
                int xb = (sym < 8 || sym == 28) ? 0 : (sym - 4) >> 2;
                if (s->nb < xb) { inf_fail(s, MPN_INFLATE_TRUNCATED); break; }
                const int len = sym == 28 ? 258 : sym < 8 ? 3 + sym : 3 + ((4 + (sym & 3)) << xb) + (int)(s->buf & ((1u << xb) - 1));
                inf_drop(s, xb);
                int dsym = inf_decode(dc, s->buf, s->nb, &l);
                if (dsym < 0) { inf_fail(s, dsym == -2 ? MPN_INFLATE_TRUNCATED : MPN_INFLATE_BAD_CODE); break; }
                inf_drop(s, l);
                if (dsym >= 30) { inf_fail(s, MPN_INFLATE_BAD_CODE); break; }
                xb = dsym < 4 ? 0 : (dsym - 2) >> 1;
                if (s->nb < xb) { inf_fail(s, MPN_INFLATE_TRUNCATED); break; }
                const int64_t dist = dsym < 4 ? 1 + dsym : 1 + ((int64_t)(2 + (dsym & 1)) << xb) + (int64_t)(s->buf & ((1u << xb) - 1));
                inf_drop(s, xb);
                if (dist > s->out_pos - s->member_start) { inf_fail(s, MPN_INFLATE_BAD_DISTANCE); break; }
                for (int k = 0; k < len; ++k) ring[(s->out_pos + k) & INF_MASK] = ring[(s->out_pos + k - dist) & INF_MASK];
                s->out_pos += len;
            }
            break;
        }
    }
}

// The flush as one thread does it (the kernel spreads the same work over a wave): ring[flushed .. out_pos) goes to
// slot[flushed ..) as far as cap allows and into the member's CRC register.
INF_HD void inf_flush_serial(InfState *s, const uint8_t *ring, uint8_t *slot, int64_t cap) {
    for (int64_t p = s->flushed; p < s->out_pos; ++p) {
        const uint8_t b = ring[p & INF_MASK];
        if (p < cap) slot[p] = b;
        s->crc = mpn_crc::crc_entry((s->crc ^ b) & 0xff) ^ (s->crc >> 8);
    }
    s->flushed = s->out_pos;
}

// The largest number of inf_run calls a stream of in_len bytes can need: a call that returns 0 has produced INF_HALF bytes
// (8 * 258 / INF_HALF < 1/7 per input byte) or finished a member (18 bytes at least).
INF_HD int64_t inf_max_calls(int64_t in_len) { return 8 + in_len / 7 + in_len / 18 + 1; }

INF_HD int inf_final_status(const InfState *s, int64_t cap) {
    return s->status == MPN_INFLATE_OK && s->out_pos > cap ? MPN_INFLATE_OVERFLOW : s->status;
}

}  // namespace mpn_inf
