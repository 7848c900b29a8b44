// BGZF block compression on the GPU behind include/mpn_bam.h (mpn_bgzf_compress): the deflate half of
// `samtools view -b | samtools sort` in the pipeline the reference starts after the species placement.  Written from RFC 1951
// (deflate), RFC 1952 (CRC-32) and SAMv1 section 4.1 (BGZF).  One workgroup of 256 lanes per BGZF block; workgroups do not talk to
// each other, nothing waits but at __syncthreads, and every loop runs to the payload length, to 258 or to a table size.
//
// Stages of bgzf_deflate_kernel (payload p[0..n), n <= 65280, stays in global memory -- L2 holds it; LDS holds tables only):
//   A  matches + greedy parse, 256 positions (one per lane) at a time: candidates are p - 1 (runs) and the last position of an
//      EARLIER tile whose next 4 bytes hash alike (8192 x u32 in LDS, ds_max per tile: the table is the same whichever lane comes
//      first); the bytes are compared, 8 at a time.  Wave 0 then walks the tile's match mask with ballots -- one step per match
//      taken, not per byte -- and every lane stores its token (literal / length + distance / nothing) at its position in a scratch
//      row in global memory and counts its symbols into the two histograms.
//   B  length-limited Huffman codes (15 / 15 / 7 bits): rank sort by all lanes, the two-queue merge on one lane, depths clamped and
//      the Kraft sum put right on the count-per-length table, lengths handed out again by rank, canonical codes bit-reversed.  As
//      zlib does, a tree with fewer than two used symbols gets symbols 0 / 1 added, so every code is complete.
//   C  the dynamic header without the run-length symbols 16-18, and the exact size of the stream from the histograms: if it is
//      not smaller than the stored form (5 + n bytes), the stored form is written.
//   D  emission: header items and tokens are one list; a wave scan + 4 wave totals place each item's bits, lanes OR them into a
//      1.6 KiB LDS window (double-buffered: two barriers per 256 items) and the window's complete bytes go to the block's slot.
//   E  CRC-32: a slice per lane with the byte table, slices joined by multiplying with x^(8 * bytes behind the slice) mod P
//      (crc32_poly.h, shared with the inflate kernel).
// Blocks land in slots of worst-case size; bgzf_scan_kernel turns the sizes into addresses and bgzf_pack_kernel moves them together.
//
// Per 65280-byte block: 64 KiB read about 3 times (match, CRC, emission) + 255 KiB of tokens written and read once: ~0.7 MB through
// L2 for 64 KiB of payload.  LDS 46 KiB per workgroup (below the 64 KiB every runtime grants; 3 workgroups share a CU).
#include "mpn_common.h"
#include "crc32_poly.h"
#include "bgzf_resident.h"
#include "../../include/mpn_bam.h"

#include <cstring>

namespace mpn {

constexpr int BZ_THREADS = 256;
constexpr int BZ_MAX_PAYLOAD = 65280;
constexpr int BZ_SLOT_EXTRA = 31;          // 18 header + 5 stored + 8 trailer: a block never needs more than its payload + 31
constexpr int BZ_HASH_BITS = 13;
constexpr int BZ_HASH_SIZE = 1 << BZ_HASH_BITS;
constexpr int BZ_WINDOW = 32768;
constexpr int BZ_TOK_STRIDE = 65536;       // tokens of one block in the scratch (u32 each)
constexpr int BZ_WIN_WORDS = 416;          // 256 items x 48 bits = 384 words + the carried byte + the 3-word reach of the last item
constexpr int BZ_NLL = 286, BZ_ND = 30, BZ_NCL = 19;
constexpr int BZ_SYM_PAD = 288;            // room for the largest alphabet
constexpr int BZ_CHUNK = 1024;             // blocks per launch (the token scratch is that many rows)

__device__ const uint8_t bz_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// length 3..258 -> symbol - 257, extra bits, extra value (RFC 1951 3.2.5)
__device__ __forceinline__ void bz_len_sym(int len, int &sym, int &nx, int &xv) {
    const int l = len - 3;
    if (len == 258) { sym = 28; nx = 0; xv = 0; return; }
    if (l < 8) { sym = l; nx = 0; xv = 0; return; }
    const int e = (31 - __clz(l)) - 2;
    sym = 4 * e + 4 + ((l >> e) & 3);
    nx = e;
    xv = l & ((1 << e) - 1);
}
// distance - 1 (0..32767) -> symbol, extra bits, extra value
__device__ __forceinline__ void bz_dist_sym(int d1, int &sym, int &nx, int &xv) {
    if (d1 < 4) { sym = d1; nx = 0; xv = 0; return; }
    const int e = (31 - __clz(d1)) - 1;
    sym = 2 * e + 2 + ((d1 >> e) & 1);
    nx = e;
    xv = d1 & ((1 << e) - 1);
}
__device__ __forceinline__ int bz_len_extra_of_sym(int s) { return (s < 8 || s == 28) ? 0 : (s - 4) >> 2; }     // s = symbol - 257
__device__ __forceinline__ int bz_dist_extra_of_sym(int s) { return s < 4 ? 0 : (s - 2) >> 1; }

// number of equal bytes of p[a..] and p[b..], at most maxl (a < b, b + maxl <= n)
__device__ __forceinline__ int bz_match_len(const uint8_t *__restrict__ p, int a, int b, int maxl) {
    int k = 0;
    while (k + 8 <= maxl) {
        uint64_t x, y;
        __builtin_memcpy(&x, p + a + k, 8);
        __builtin_memcpy(&y, p + b + k, 8);
        const uint64_t d = x ^ y;
        if (d) return k + ((__ffsll((unsigned long long)d) - 1) >> 3);
        k += 8;
    }
    while (k < maxl && p[a + k] == p[b + k]) ++k;
    return k;
}

struct BzShared {
    uint32_t head[BZ_HASH_SIZE];          // hash -> 1 + last position of an earlier tile, 0 = none
    uint32_t win[2][BZ_WIN_WORDS];
    uint32_t crc_tab[256];
    uint32_t hist_ll[BZ_SYM_PAD], hist_d[32], hist_cl[32];
    uint32_t f2[BZ_SYM_PAD], w[BZ_SYM_PAD], iw[BZ_SYM_PAD];
    uint16_t srt[BZ_SYM_PAD], lpar[BZ_SYM_PAD], ipar[BZ_SYM_PAD], idep[BZ_SYM_PAD];
    uint16_t code_ll[BZ_SYM_PAD], code_d[32], code_cl[32];
    uint8_t len_ll[BZ_SYM_PAD], len_d[32], len_cl[32];
    uint16_t mlen[BZ_THREADS];
    unsigned long long smask[4];
    int blc[16], first_rank[17];
    uint32_t next_code[16];
    int wtot[4];
    int used, hlit, hdist, hclen;
    uint32_t bits, crc;
};

// Length-limited canonical Huffman code of freq[0..nsym): lens[] (0 = unused) and the bit-reversed codes[].  All lanes call it.
__device__ void bz_build_code(BzShared &s, const uint32_t *freq, int nsym, int maxbits, uint8_t *lens, uint16_t *codes) {
    const int tid = threadIdx.x;
    if (tid == 0) s.used = 0;
    if (tid < 16) s.blc[tid] = 0;
    __syncthreads();
    for (int k = tid; k < nsym; k += BZ_THREADS) { s.f2[k] = freq[k]; lens[k] = 0; if (freq[k]) atomicAdd(&s.used, 1); }
    __syncthreads();
    if (tid == 0 && s.used < 2) {     // zlib's rule: at least two codes of non-zero frequency
        if (s.used == 0) { s.f2[0] = 1; s.f2[1] = 1; }
        else if (s.f2[0]) s.f2[1] = 1;
        else s.f2[0] = 1;
        s.used = 2;
    }
    __syncthreads();
    const int m = s.used;
    // rank of every used symbol by (frequency, symbol)
    for (int k = tid; k < nsym; k += BZ_THREADS) {
        const uint32_t f = s.f2[k];
        if (!f) continue;
        int r = 0;
        for (int j = 0; j < nsym; ++j) { const uint32_t g = s.f2[j]; r += (g && (g < f || (g == f && j < k))) ? 1 : 0; }
        s.srt[r] = (uint16_t)k;
        s.w[r] = f;
    }
    __syncthreads();
    if (tid == 0) {   // two-queue merge over the sorted leaves: m - 1 internal nodes, created in ascending weight
        int li = 0, ii = 0;
        for (int nn = 0; nn < m - 1; ++nn) {
            uint32_t sum = 0;
            for (int c = 0; c < 2; ++c) {
                if (li < m && (ii >= nn || s.w[li] <= s.iw[ii])) { sum += s.w[li]; s.lpar[li++] = (uint16_t)nn; }
                else { sum += s.iw[ii]; s.ipar[ii++] = (uint16_t)nn; }
            }
            s.iw[nn] = sum;
        }
        s.idep[m - 2] = 0;
        for (int k = m - 3; k >= 0; --k) s.idep[k] = s.idep[s.ipar[k]] + 1;
    }
    __syncthreads();
    for (int r = tid; r < m; r += BZ_THREADS) {
        int d = s.idep[s.lpar[r]] + 1;
        if (d > maxbits) d = maxbits;
        atomicAdd(&s.blc[d], 1);
    }
    __syncthreads();
    if (tid == 0) {
        // Kraft sum in units of 2^-maxbits: clamping can only have made it too large
        const int full = 1 << maxbits;
        int K = 0;
        for (int l = 1; l <= maxbits; ++l) K += s.blc[l] << (maxbits - l);
        for (int it = 0; it < BZ_SYM_PAD && K > full; ++it) {     // lengthen the longest code that is not at the limit
            int l = maxbits - 1;
            while (l > 0 && s.blc[l] == 0) --l;
            if (l == 0) break;
            --s.blc[l]; ++s.blc[l + 1];
            K -= 1 << (maxbits - l - 1);
        }
        for (int it = 0; it < full && K < full; ++it) {           // hand back what the last step took too much: shorten one code
            const int D = full - K;
            int l = 1;
            while (l <= maxbits && (s.blc[l] == 0 || (1 << (maxbits - l)) > D)) ++l;
            if (l > maxbits) break;
            --s.blc[l]; ++s.blc[l - 1];
            K += 1 << (maxbits - l);
        }
        // ranks ascend with frequency: the rarest symbols take the longest codes
        int r = 0;
        for (int l = maxbits; l >= 1; --l) { s.first_rank[l] = r; r += s.blc[l]; }
        s.first_rank[0] = r;
        uint32_t code = 0;
        s.next_code[0] = 0;
        for (int l = 1; l <= maxbits; ++l) { code = (code + (l > 1 ? s.blc[l - 1] : 0)) << 1; s.next_code[l] = code; }
    }
    __syncthreads();
    for (int r = tid; r < m; r += BZ_THREADS) {
        int l = maxbits;
        while (l > 1 && r >= s.first_rank[l] + s.blc[l]) --l;
        lens[s.srt[r]] = (uint8_t)l;
    }
    __syncthreads();
    for (int k = tid; k < nsym; k += BZ_THREADS) {
        const int l = lens[k];
        if (!l) { codes[k] = 0; continue; }
        uint32_t c = s.next_code[l];
        for (int j = 0; j < k; ++j) c += lens[j] == l ? 1 : 0;
        codes[k] = (uint16_t)(__brev(c) >> (32 - l));
    }
    __syncthreads();
}

__global__ __launch_bounds__(BZ_THREADS) void bgzf_deflate_kernel(const uint8_t *__restrict__ payload, const int64_t *__restrict__ pay_off,
                                                                  int64_t first_block, uint8_t *__restrict__ slots, uint32_t *__restrict__ tok_all,
                                                                  int32_t *__restrict__ sizes, int mode) {
    __shared__ BzShared s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = first_block + blockIdx.x;
    const int64_t o0 = pay_off[blk];
    const int n = (int)(pay_off[blk + 1] - o0);
    const uint8_t *__restrict__ p = payload + (o0 - pay_off[0]);     // the device copy of the payload starts at pay_off[0]
    uint8_t *__restrict__ slot = slots + (o0 - pay_off[0]) + (int64_t)BZ_SLOT_EXTRA * blk;
    uint8_t *__restrict__ dst = slot + 18;
    uint32_t *__restrict__ tok = tok_all + (size_t)blockIdx.x * BZ_TOK_STRIDE;

    for (int k = tid; k < BZ_HASH_SIZE; k += BZ_THREADS) s.head[k] = 0;
    for (int k = tid; k < BZ_WIN_WORDS; k += BZ_THREADS) { s.win[0][k] = 0; s.win[1][k] = 0; }
    for (int k = tid; k < BZ_SYM_PAD; k += BZ_THREADS) s.hist_ll[k] = 0;
    if (tid < 32) { s.hist_d[tid] = 0; s.hist_cl[tid] = 0; }
    s.crc_tab[tid] = mpn_crc::crc_entry((uint32_t)tid);
    if (tid == 0) { s.bits = 0; s.crc = 0; s.hlit = 257; s.hdist = 1; }
    __syncthreads();

    // ---- E: CRC-32 (needed by every mode) ----
    {
        const int per = (n + BZ_THREADS - 1) / BZ_THREADS;
        const int a = min(n, tid * per), b = min(n, a + per);
        uint32_t c = 0;
        for (int k = a; k < b; ++k) c = s.crc_tab[(c ^ p[k]) & 0xff] ^ (c >> 8);
        uint32_t part = mpn_crc::crc_slice(c, (uint32_t)(n - b));
        if (tid == 0) part = mpn_crc::crc_join(0xFFFFFFFFu, (uint32_t)n, part);     // the register a member starts with
        atomicXor(&s.crc, part);
    }

    bool stored = mode == MPN_BGZF_STORED;
    int dyn_bytes = 0;
    uint32_t total_bits = 0;
    if (!stored) {
        // ---- A: matches, greedy parse, histograms ----
        int next_tok = 0;     // wave 0: the position where the next token starts
        const int n_tiles = (n + BZ_THREADS - 1) / BZ_THREADS;
        for (int tile = 0; tile < n_tiles; ++tile) {
            const int pos = tile * BZ_THREADS + tid;
            int L = 0, D = 0;
            uint32_t h = 0;
            bool has_h = false;
            if (pos < n) {
                L = 1;
                const int maxl = min(258, n - pos);
                if (mode == MPN_BGZF_AUTO && maxl >= 3) {
                    if (pos >= 1) { const int l0 = bz_match_len(p, pos - 1, pos, maxl); if (l0 >= 3) { L = l0; D = 1; } }
                    if (maxl >= 4) {
                        uint32_t w4;
                        __builtin_memcpy(&w4, p + pos, 4);
                        h = (w4 * 2654435761u) >> (32 - BZ_HASH_BITS);
                        has_h = true;
                        const uint32_t c = s.head[h];
                        if (c && L < maxl) {
                            const int cand = (int)c - 1, d1 = pos - cand;      // cand lies in an earlier tile: cand < pos
                            if (d1 <= BZ_WINDOW) {
                                const int l1 = bz_match_len(p, cand, pos, maxl);
                                // a 4-byte match far back costs more bits than four literals of any skewed alphabet
                                if (l1 > L && (l1 >= 5 || (l1 == 4 && d1 < 4096))) { L = l1; D = d1; }
                            }
                        }
                    }
                }
            }
            s.mlen[tid] = (uint16_t)L;
            __syncthreads();
            if (has_h) atomicMax(&s.head[h], (uint32_t)pos + 1);
            if (wave == 0) {
                for (int wq = 0; wq < 4; ++wq) {
                    const int base = tile * BZ_THREADS + wq * 64;
                    const int Lw = s.mlen[wq * 64 + lane];
                    const unsigned long long M = __ballot(Lw >= 3);
                    unsigned long long S = 0;
                    int q = next_tok > base ? next_tok - base : 0;
                    for (int it = 0; it < 64 && q < 64; ++it) {      // every step but the last passes a match of 3 or more
                        const unsigned long long rem = M & (~0ull << q);
                        if (!rem) { S |= ~0ull << q; q = 64; break; }
                        const int mpos = __ffsll(rem) - 1;
                        S |= (~0ull << q) & ((2ull << mpos) - 1);
                        q = mpos + __shfl(Lw, mpos);
                    }
                    next_tok = base + q;
                    if (lane == 0) s.smask[wq] = S;
                }
            }
            __syncthreads();
            if (pos < n) {
                uint32_t t = 0;
                if ((s.smask[wave] >> lane) & 1) {
                    if (L >= 3) {
                        t = (uint32_t)L | (uint32_t)(D - 1) << 16;
                        int sym, nx, xv;
                        bz_len_sym(L, sym, nx, xv);
                        atomicAdd(&s.hist_ll[257 + sym], 1u);
                        bz_dist_sym(D - 1, sym, nx, xv);
                        atomicAdd(&s.hist_d[sym], 1u);
                    } else {
                        t = 1;
                        atomicAdd(&s.hist_ll[p[pos]], 1u);
                    }
                }
                tok[pos] = t;
            }
        }
        if (tid == 0) s.hist_ll[256] = 1;

        // ---- B: the three codes ----
        bz_build_code(s, s.hist_ll, BZ_NLL, 15, s.len_ll, s.code_ll);
        bz_build_code(s, s.hist_d, BZ_ND, 15, s.len_d, s.code_d);
        for (int k = tid; k < BZ_NLL; k += BZ_THREADS) if (s.len_ll[k]) atomicMax(&s.hlit, k + 1);
        if (tid < BZ_ND && s.len_d[tid]) atomicMax(&s.hdist, tid + 1);
        __syncthreads();
        const int hlit = s.hlit, hdist = s.hdist;
        for (int k = tid; k < hlit + hdist; k += BZ_THREADS) atomicAdd(&s.hist_cl[k < hlit ? s.len_ll[k] : s.len_d[k - hlit]], 1u);
        bz_build_code(s, s.hist_cl, BZ_NCL, 7, s.len_cl, s.code_cl);

        // ---- C: header shape and the exact size ----
        if (tid == 0) {
            int hc = 19;
            while (hc > 4 && s.len_cl[bz_cl_order[hc - 1]] == 0) --hc;
            s.hclen = hc;
            atomicAdd(&s.bits, 17u + 3u * (uint32_t)hc);
        }
        {
            uint32_t b = 0;
            for (int k = tid; k < BZ_NLL; k += BZ_THREADS) b += s.hist_ll[k] * (s.len_ll[k] + (k > 256 ? bz_len_extra_of_sym(k - 257) : 0));
            if (tid < BZ_ND) b += s.hist_d[tid] * (s.len_d[tid] + bz_dist_extra_of_sym(tid));
            if (tid < BZ_NCL) b += s.hist_cl[tid] * s.len_cl[tid];
            if (b) atomicAdd(&s.bits, b);
        }
        __syncthreads();
        total_bits = s.bits;
        dyn_bytes = (int)((total_bits + 7) >> 3);
        stored = dyn_bytes >= 5 + n;
    }

    int body;
    bool bad = false;
    if (stored) {
        body = 5 + n;
        if (tid == 0) { dst[0] = 1; dst[1] = (uint8_t)n; dst[2] = (uint8_t)(n >> 8); dst[3] = (uint8_t)~n; dst[4] = (uint8_t)(~n >> 8); }
        for (int k = tid; k < n; k += BZ_THREADS) dst[5 + k] = p[k];
    } else {
        // ---- D: emission ----
        body = dyn_bytes;
        const int hlit = s.hlit, hdist = s.hdist, hclen = s.hclen;
        const int H = 1 + hclen + hlit + hdist, total_items = H + n + 1;
        uint32_t base_bits = 0, carry = 0;
        int cur = 0;
        for (int i0 = 0; i0 < total_items; i0 += BZ_THREADS) {
            const int idx = i0 + tid;
            uint64_t val = 0;
            int nb = 0;
            if (idx < total_items) {
                if (idx >= H) {
                    const int pos = idx - H;
                    if (pos == n) { val = s.code_ll[256]; nb = s.len_ll[256]; }
                    else {
                        const uint32_t t = tok[pos];
                        const int L = (int)(t & 0x1ff);
                        if (L == 1) { const int c = p[pos]; val = s.code_ll[c]; nb = s.len_ll[c]; }
                        else if (L >= 3) {
                            int sym, nx, xv;
                            bz_len_sym(L, sym, nx, xv);
                            val = s.code_ll[257 + sym]; nb = s.len_ll[257 + sym];
                            val |= (uint64_t)xv << nb; nb += nx;
                            bz_dist_sym((int)(t >> 16), sym, nx, xv);
                            val |= (uint64_t)s.code_d[sym] << nb; nb += s.len_d[sym];
                            val |= (uint64_t)xv << nb; nb += nx;
                        }
                    }
                } else if (idx == 0) { val = 5u | (uint32_t)(hlit - 257) << 3 | (uint32_t)(hdist - 1) << 8 | (uint32_t)(hclen - 4) << 13; nb = 17; }
                else if (idx <= hclen) { val = s.len_cl[bz_cl_order[idx - 1]]; nb = 3; }
                else {
                    const int k = idx - 1 - hclen;
                    const int v = k < hlit ? s.len_ll[k] : s.len_d[k - hlit];
                    val = s.code_cl[v]; nb = s.len_cl[v];
                }
            }
            const int incl = wave_scan_add(nb);
            if (lane == 63) s.wtot[wave] = incl;
            __syncthreads();
            int woff = 0, ttot = 0;
            for (int k = 0; k < 4; ++k) { const int v = s.wtot[k]; ttot += v; woff += k < wave ? v : 0; }
            const uint32_t origin = base_bits & ~7u;
            if (nb) {
                const uint32_t rel = base_bits + (uint32_t)(woff + incl - nb) - origin;
                const int w0 = (int)(rel >> 5), sh = (int)(rel & 31);
                const uint64_t lo = val << sh;
                const uint32_t v0 = (uint32_t)lo, v1 = (uint32_t)(lo >> 32), v2 = sh ? (uint32_t)(val >> (64 - sh)) : 0;
                if (v0) atomicOr(&s.win[cur][w0], v0);
                if (v1) atomicOr(&s.win[cur][w0 + 1], v1);
                if (v2) atomicOr(&s.win[cur][w0 + 2], v2);
            }
            if (tid == 0 && carry) atomicOr(&s.win[cur][0], carry);
            __syncthreads();
            const uint32_t end = base_bits + (uint32_t)ttot;
            const int cb = (int)((end >> 3) - (origin >> 3));
            const uint8_t *winb = (const uint8_t *)s.win[cur];
            for (int k = tid; k < cb; k += BZ_THREADS) {
                const int o = (int)(origin >> 3) + k;
                if (o < dyn_bytes) dst[o] = winb[k];
            }
            if (tid == 0) carry = (end & 7) ? winb[cb] : 0;
            for (int k = tid; k < BZ_WIN_WORDS; k += BZ_THREADS) s.win[cur ^ 1][k] = 0;
            base_bits = end;
            cur ^= 1;
        }
        if (tid == 0 && (base_bits & 7) && (int)(base_bits >> 3) < dyn_bytes) dst[base_bits >> 3] = (uint8_t)carry;
        bad = base_bits != total_bits;     // the size from the histograms and the bits placed must agree
    }
    __syncthreads();
    if (tid == 0) {
        const int total = 18 + body + 8;
        const uint8_t hd[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        for (int k = 0; k < 16; ++k) slot[k] = hd[k];
        slot[16] = (uint8_t)(total - 1);
        slot[17] = (uint8_t)((total - 1) >> 8);
        const uint32_t crc = s.crc ^ 0xFFFFFFFFu;
        uint8_t *tr = slot + 18 + body;
        for (int k = 0; k < 4; ++k) { tr[k] = (uint8_t)(crc >> (8 * k)); tr[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
        sizes[blk] = bad ? -1 : total;
    }
}

// one block: out_off[i] = the sizes before block i, out_off[n] = all of them; flag[0] = 1 if a block reported an inconsistency
__global__ __launch_bounds__(1024) void bgzf_scan_kernel(const int32_t *__restrict__ sizes, int64_t n, int64_t *__restrict__ out_off, int *__restrict__ flag) {
    __shared__ int64_t part[1024];
    __shared__ int any_bad;
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    if (t == 0) any_bad = 0;
    __syncthreads();
    int64_t sum = 0;
    for (int64_t k = lo; k < hi; ++k) { if (sizes[k] < 0) any_bad = 1; else sum += sizes[k]; }
    part[t] = sum;
    __syncthreads();
    if (t == 0) { int64_t acc = 0; for (int k = 0; k < 1024; ++k) { const int64_t v = part[k]; part[k] = acc; acc += v; } out_off[n] = acc; flag[0] = any_bad; }
    __syncthreads();
    int64_t o = part[t];
    for (int64_t k = lo; k < hi; ++k) { out_off[k] = o; o += sizes[k] < 0 ? 0 : sizes[k]; }
}

// one workgroup per block: slot -> its place in the packed output
__global__ __launch_bounds__(BZ_THREADS) void bgzf_pack_kernel(const uint8_t *__restrict__ slots, const int64_t *__restrict__ pay_off,
                                                               const int64_t *__restrict__ out_off, uint8_t *__restrict__ out) {
    const int64_t blk = blockIdx.x;
    const uint8_t *__restrict__ src = slots + (pay_off[blk] - pay_off[0]) + (int64_t)BZ_SLOT_EXTRA * blk;
    uint8_t *__restrict__ d = out + out_off[blk];
    const int len = (int)(out_off[blk + 1] - out_off[blk]);
    for (int k = threadIdx.x; k < len; k += BZ_THREADS) d[k] = src[k];
}

thread_local double tl_bgzf_ms[2] = {0, 0};   // device time of the last call on this thread: deflate + scan, pack

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_bgzf_last_device_ms(double *deflate_ms, double *pack_ms) {
    if (deflate_ms) *deflate_ms = tl_bgzf_ms[0];
    if (pack_ms) *pack_ms = tl_bgzf_ms[1];
}

extern "C" int64_t mpn_bgzf_compress(int64_t n_blocks, const uint8_t *payload, const int64_t *pay_off, uint8_t *out, int64_t out_cap,
                                     int64_t *out_off, int32_t mode) {
    if (n_blocks < 0 || !pay_off || !out_off || out_cap < 0 || (out_cap > 0 && !out) || mode < MPN_BGZF_AUTO || mode > MPN_BGZF_NO_MATCH ||
        n_blocks > 0x7fffffff) {
        set_error("mpn_bgzf_compress: bad arguments");
        return -2;
    }
    for (int64_t i = 0; i < n_blocks; ++i) {
        const int64_t len = pay_off[i + 1] - pay_off[i];
        if (len < 0 || len > BZ_MAX_PAYLOAD) {
            set_error("mpn_bgzf_compress: block %lld has %lld payload bytes (0..%d allowed)", (long long)i, (long long)len, BZ_MAX_PAYLOAD);
            return -1;
        }
    }
    out_off[0] = 0;
    if (n_blocks == 0) return 0;
    const int64_t pay_bytes = pay_off[n_blocks] - pay_off[0];
    if (pay_bytes > 0 && !payload) { set_error("mpn_bgzf_compress: bad arguments"); return -2; }
    hipStream_t st = 0;
    DevBuf<uint8_t> d_pay;
    DevBuf<int64_t> d_po;
    BgzfWork w;
    DevTimer tm_pack;
    tl_bgzf_ms[0] = tl_bgzf_ms[1] = 0;
    if (d_pay.upload(payload + pay_off[0], (size_t)pay_bytes, st) || d_po.upload(pay_off, (size_t)n_blocks + 1, st)) return -1;
    const int64_t total = bgzf_deflate_resident(d_pay.p, pay_bytes, d_po.p, n_blocks, mode, st, w, out_off);
    if (total < 0) return -1;
    if (total > out_cap) { set_error("mpn_bgzf_compress: out_cap %lld is below the %lld bytes needed", (long long)out_cap, (long long)total); return -3; }
    if (bgzf_pack_resident(d_po.p, n_blocks, total, st, w, tm_pack)) return -1;
    if (w.out.download(out, (size_t)total, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (tm_pack.elapsed_ms(&tl_bgzf_ms[1])) return -1;
    return total;
}

int64_t mpn::bgzf_deflate_resident(const uint8_t *d_pay, int64_t pay_bytes, const int64_t *d_po, int64_t n_blocks, int32_t mode, hipStream_t st,
                                   BgzfWork &w, int64_t *out_off) {
    const int64_t chunk = std::min<int64_t>(n_blocks, BZ_CHUNK);
    DevTimer tm_deflate;
    if (w.slots.alloc((size_t)(pay_bytes + BZ_SLOT_EXTRA * n_blocks)) || w.oo.alloc((size_t)n_blocks + 1) || w.sizes.alloc((size_t)n_blocks) ||
        w.flag.alloc(1) || (mode != MPN_BGZF_STORED && w.tok.alloc((size_t)chunk * BZ_TOK_STRIDE)) || tm_deflate.start(st))
        return -1;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += chunk) {   // launches on one stream run one after another: they share the token rows
        const int g = (int)std::min<int64_t>(chunk, n_blocks - b0);
        hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(g), dim3(BZ_THREADS), 0, st, d_pay, d_po, b0, w.slots.p, w.tok.p, w.sizes.p, (int)mode);
    }
    hipLaunchKernelGGL(bgzf_scan_kernel, dim3(1), dim3(1024), 0, st, (const int32_t *)w.sizes.p, n_blocks, w.oo.p, w.flag.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm_deflate.stop(st)) return -1;
    int flag = 0;
    if (w.oo.download(out_off, (size_t)n_blocks + 1, st) || w.flag.download(&flag, 1, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (tm_deflate.elapsed_ms(&tl_bgzf_ms[0])) return -1;
    if (flag) { set_error("mpn_bgzf_compress: a block's emitted bits disagree with its computed size"); return -1; }
    return out_off[n_blocks];
}

int mpn::bgzf_pack_resident(const int64_t *d_po, int64_t n_blocks, int64_t total, hipStream_t st, BgzfWork &w, DevTimer &tm) {
    if (w.out.alloc((size_t)total) || tm.start(st)) return -1;
    hipLaunchKernelGGL(bgzf_pack_kernel, dim3((unsigned)n_blocks), dim3(BZ_THREADS), 0, st, (const uint8_t *)w.slots.p, d_po, (const int64_t *)w.oo.p, w.out.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    return 0;
}
