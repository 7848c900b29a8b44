// BAM files as read input, behind include/mpn_ingest.h: the BGZF blocks of the file have been inflated into slots by
// mpn_gzip_inflate_device; here their text is made contiguous, its records are found and the reads are decoded into the layout of
// mapper.PackedReads.from_arrays.  Semantics: `samtools fastq`.
//
//   bam_flatten_kernel   slots (16-byte aligned, gaps between them) + the tail the group before left -> one text.  A chunked
//                        gather like split_gather_kernel (read_split_kernels.hip), on the pieces of gather16.h: a wave owns an
//                        aligned MPN_BAM_CHUNK of the OUTPUT, a lane 16 bytes of it; every store is one aligned 16-byte store and
//                        every output byte is written once.
//   bam_walk_kernel      one wave.  The record starts are a dependent chain through block_size: lane 0 follows it for 64 records
//                        (one 4-byte read per record: bam_walk_core.h bamw_step), then the 64 lanes read the fixed fields of
//                        those records side by side and store a 16-byte row each (bamw_row).  Stops at the first record that is
//                        malformed or passes the end.
//   bam_prep_kernel      a thread per kept record: where its packed bases start (name and CIGAR skipped), the check that bases and
//                        qualities lie inside the text, and its name into the pool (as fa_names_kernel does).
//   bam_decode_kernel    the hot path.  As in the gather a wave owns an aligned chunk of the output buffers, and chunk_rec (the CSR
//                        of records per chunk, made on the host) says which records touch it: the work is bounded in bytes, a
//                        200 kb read is spread over two hundred wave steps.  A lane whose 16 output bytes lie in one read turns 8
//                        packed bytes (9 when its first base is the second of a byte) into 16 ASCII bases and 16 Phred bytes into
//                        Phred+33; a reverse read is taken from the mirrored position, nibbles and bytes in the opposite order,
//                        through the complement table.  Lanes at a read's head or tail go byte by byte.
// No atomics anywhere; the only flag (a row that does not fit the text) is a plain store of one value.
#include "gather16.h"
#include "bam_walk_core.h"

#include <string.h>

namespace mpn {

using namespace mpn_bamw;

thread_local double tl_bam_ms[3] = {0, 0, 0};   // device time of the last calls on this thread: flatten, walk, decode

static_assert(sizeof(mpn_bam_row) == 16, "a row is one 16-byte store");

// ---- flatten -------------------------------------------------------------------------------------------------------------------
// Segment j: seg_len[j] > 0 bytes from the address seg_src[j] to text[seg_dst[j] ..); seg_dst ascending, the segments back to back
// from 0 to text_len.  out_bytes: text_len rounded up to 16.
__global__ __launch_bounds__(G16_THREADS) void bam_flatten_kernel(const int64_t *__restrict__ seg_dst, const int64_t *__restrict__ seg_src,
                                                                  const int64_t *__restrict__ seg_len, int64_t n_seg, uint8_t *__restrict__ text,
                                                                  int64_t out_bytes) {
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (out_bytes + MPN_BAM_CHUNK - 1) / MPN_BAM_CHUNK;
    for (int64_t c = (int64_t)blockIdx.x * G16_WAVES + (threadIdx.x >> 6); c < n_chunks; c += (int64_t)gridDim.x * G16_WAVES) {
        const int64_t c0 = c * MPN_BAM_CHUNK;
        const int64_t c1 = (c0 + MPN_BAM_CHUNK < out_bytes ? c0 + MPN_BAM_CHUNK : out_bytes) - 1;
        // wave-uniform: the segments that can cover bytes of [c0, c1] (seg_dst[0] = 0, so jlo >= 0)
        const int64_t jlo = last_le(seg_dst, 0, n_seg - 1, c0), jhi = last_le(seg_dst, jlo, n_seg - 1, c1);
        const int64_t p = c0 + lane * 16;
        if (p >= out_bytes) continue;
        const int64_t j = last_le(seg_dst, jlo, jhi, p);
        const int64_t d = seg_dst[j], l = seg_len[j];
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p + 16 <= d + l) {
            v = load16((const uint8_t *)(uintptr_t)seg_src[j] + (p - d));
        } else {
            // the end of a segment, short segments, or the padding behind the text: byte by byte
            uint32_t w[4] = {0, 0, 0, 0};
            int64_t jj = j;
#pragma unroll 1
            for (int b = 0; b < 16; ++b) {
                const int64_t q = p + b;
                jj = last_le(seg_dst, jj, jhi, q);
                const int64_t dd = seg_dst[jj];
                uint32_t byte = 0;
                if (q < dd + seg_len[jj]) byte = ((const uint8_t *)(uintptr_t)seg_src[jj])[q - dd];
                w[b >> 2] |= byte << (8 * (b & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4 *)(text + p) = v;
    }
}

// ---- walk ----------------------------------------------------------------------------------------------------------------------
// res[0] = records, res[1] = next, res[2] = status.  rows has room for max_records.
__global__ __launch_bounds__(64) void bam_walk_kernel(const uint8_t *__restrict__ text, int64_t len, int64_t start, int at_header, int final_call,
                                                      int64_t max_records, mpn_bam_row *__restrict__ rows, int64_t *__restrict__ res) {
    __shared__ int64_t s_off[65];    // the starts of this round's records and the end of the last one
    __shared__ int64_t s_pos;
    __shared__ int s_cnt, s_stop;    // s_stop: BAMW_WHOLE = go on, otherwise why the chain ended
    __shared__ int32_t s_status;
    const int lane = threadIdx.x;
    if (lane == 0) {
        int64_t pos = start;
        int32_t status = MPN_INFLATE_OK;
        int stop = BAMW_WHOLE;
        if (at_header) stop = bamw_header(text, len, start, &pos, &status);
        s_pos = pos; s_stop = stop; s_status = status;
    }
    __syncthreads();
    int64_t n = 0;
    // a round takes up to 64 records; every round but the last takes 64, so the rounds are bounded by max_records
    while (s_stop == BAMW_WHOLE && n < max_records) {
        if (lane == 0) {
            const int want = (int)min((int64_t)64, max_records - n);
            int64_t off = s_pos;
            int cnt = 0, stop = BAMW_WHOLE;
            while (cnt < want) {
                int64_t end = 0;
                stop = bamw_step(text, len, off, &end);
                if (stop != BAMW_WHOLE) break;
                s_off[cnt++] = off;
                off = end;
            }
            s_off[cnt] = off;
            s_cnt = cnt; s_stop = stop;
        }
        __syncthreads();
        const int cnt = s_cnt;
        mpn_bam_row row;
        const bool bad = lane < cnt && bamw_row(text, s_off[lane], s_off[lane + 1], &row) != 0;
        const unsigned long long bad_mask = __ballot(bad);
        const int good = bad_mask ? __ffsll(bad_mask) - 1 : cnt;
        if (lane < good) rows[n + lane] = row;
        n += good;
        __syncthreads();       // s_off and s_stop have been read before lane 0 writes them again
        if (lane == 0) {
            s_pos = s_off[good];
            if (good < cnt) s_stop = BAMW_BAD;
        }
        __syncthreads();
    }
    if (lane == 0) {
        int32_t status = s_status;
        const int stop = s_stop;
        if (status == MPN_INFLATE_OK) {
            if (stop == BAMW_BAD) status = MPN_BAM_BAD_RECORD;
            else if (stop == BAMW_PARTIAL && final_call) status = MPN_BAM_TRUNCATED;
        }
        res[0] = n; res[1] = s_pos; res[2] = status;
    }
}

// ---- decode --------------------------------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) BamRec { int64_t seq; int32_t l_seq; uint32_t bits; };   // bits: 1 reverse, 2 qualities, 4 outside the text
constexpr uint32_t BR_REV = 1, BR_QUAL = 2, BR_OUT = 4;

// thread per record: rows -> recs, names -> pool; *bad = 1 if a row does not lie in the text
__global__ __launch_bounds__(256) void bam_prep_kernel(const uint8_t *__restrict__ text, int64_t text_len, const mpn_bam_row *__restrict__ rows,
                                                       const int64_t *__restrict__ pool_off, int64_t n, BamRec *__restrict__ recs,
                                                       uint8_t *__restrict__ pool, int32_t *__restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const mpn_bam_row row = rows[r];      // (the host has checked: off >= 0, off + 36 <= text_len, l_seq >= 0, l_read_name >= 1)
    BamRec rec;
    rec.seq = bamw_seq_off(text, &row);
    rec.l_seq = row.l_seq;
    rec.bits = ((row.flag & 0x10) ? BR_REV : 0) | (row.has_qual ? BR_QUAL : 0);
    if (rec.seq + ((int64_t)row.l_seq + 1) / 2 + row.l_seq > text_len) {
        rec.bits = BR_OUT; rec.l_seq = row.l_seq; rec.seq = 0;
        *bad = 1;
    } else {
        const uint8_t *__restrict__ p = text + row.off + BAMW_FIXED;
        uint8_t *__restrict__ d = pool + pool_off[r];
        for (int k = 0; k + 1 < row.l_read_name; ++k) d[k] = p[k];
    }
    recs[r] = rec;
}

constexpr uint64_t bi_pack8(const char *s) {
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) v |= (uint64_t)(uint8_t)s[k] << (8 * k);
    return v;
}
// nibble -> base, and nibble -> the base of the complement (the complement of a code is its four bits in the opposite order)
constexpr uint64_t BI_FWD_LO = bi_pack8("=ACMGRSV"), BI_FWD_HI = bi_pack8("TWYHKDBN");
constexpr uint64_t BI_REV_LO = bi_pack8("=TGKCYSB"), BI_REV_HI = bi_pack8("AWRDMHVN");

__device__ __forceinline__ uint32_t bi_base(uint32_t nib, bool rev) {
    const uint64_t t = (nib & 8) ? (rev ? BI_REV_HI : BI_FWD_HI) : (rev ? BI_REV_LO : BI_FWD_LO);
    return (uint32_t)(t >> ((nib & 7) * 8)) & 0xffu;
}
// four bytes + 33 each, mod 256, no carry from byte to byte
__device__ __forceinline__ uint32_t bi_add33(uint32_t x) { return ((x & 0x7f7f7f7fu) + 0x21212121u) ^ (x & 0x80808080u); }

__global__ __launch_bounds__(G16_THREADS) void bam_decode_kernel(const uint8_t *__restrict__ text, const BamRec *__restrict__ recs,
                                                                 const int64_t *__restrict__ out_off, const int32_t *__restrict__ chunk_rec,
                                                                 int64_t out_bytes, uint8_t *__restrict__ d_seq, uint8_t *__restrict__ d_qual) {
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (out_bytes + MPN_BAM_CHUNK - 1) / MPN_BAM_CHUNK;
    for (int64_t c = (int64_t)blockIdx.x * G16_WAVES + (threadIdx.x >> 6); c < n_chunks; c += (int64_t)gridDim.x * G16_WAVES) {
        // wave-uniform: the records that can cover bytes of the chunk (out_off[0] = 0, so the first of them is >= 0)
        const int64_t jlo = chunk_rec[c], jhi = chunk_rec[c + 1];
        const int64_t p = c * MPN_BAM_CHUNK + lane * 16;
        if (p >= out_bytes) continue;   // (out_bytes is a multiple of 16)
        const int64_t j = last_le(out_off, jlo, jhi, p);
        const int64_t d = out_off[j];
        const BamRec r = recs[j];
        uint4 vs = make_uint4(0, 0, 0, 0), vq = make_uint4(0, 0, 0, 0);
        if (p + 16 <= d + r.l_seq && !(r.bits & BR_OUT)) {
            // all 16 bytes inside read j: bases [lo, lo + 16) of the record, ascending for a forward read, descending for a reverse one
            const bool rev = r.bits & BR_REV;
            const int64_t i = p - d, lo = rev ? (int64_t)r.l_seq - 16 - i : i;
            const uint8_t *__restrict__ sp = text + r.seq + (lo >> 1);
            uint64_t w;
            memcpy(&w, sp, 8);
            // a byte holds the earlier base in its high nibble: swap the nibbles of every byte, and base k of the 16 is nibble k
            w = ((w & 0x0f0f0f0f0f0f0f0full) << 4) | ((w >> 4) & 0x0f0f0f0f0f0f0f0full);
            if (lo & 1) w = (w >> 4) | ((uint64_t)(sp[8] >> 4) << 60);      // (the ninth byte holds base lo + 15: inside the field)
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const uint32_t nib = (uint32_t)(w >> (4 * (rev ? 15 - t : t))) & 15u;
                o[t >> 2] |= bi_base(nib, rev) << (8 * (t & 3));
            }
            vs = make_uint4(o[0], o[1], o[2], o[3]);
            if (d_qual) {
                if (r.bits & BR_QUAL) {
                    const uint4 q = load16(text + r.seq + (((int64_t)r.l_seq + 1) >> 1) + lo);
                    const uint32_t a0 = bi_add33(q.x), a1 = bi_add33(q.y), a2 = bi_add33(q.z), a3 = bi_add33(q.w);
                    vq = rev ? make_uint4(__builtin_bswap32(a3), __builtin_bswap32(a2), __builtin_bswap32(a1), __builtin_bswap32(a0))
                             : make_uint4(a0, a1, a2, a3);
                } else {
                    vq = make_uint4(0x21212121u, 0x21212121u, 0x21212121u, 0x21212121u);
                }
            }
        } else {
            // the head or the tail of a read, short reads, or the padding behind the last one: byte by byte
            uint32_t ws[4] = {0, 0, 0, 0}, wq[4] = {0, 0, 0, 0};
            int64_t jj = j;
#pragma unroll 1
            for (int b = 0; b < 16; ++b) {
                const int64_t q = p + b;
                jj = last_le(out_off, jj, jhi, q);
                const BamRec rr = recs[jj];
                const int64_t k = q - out_off[jj];
                if (k >= rr.l_seq || (rr.bits & BR_OUT)) continue;
                const bool rev = rr.bits & BR_REV;
                const int64_t src = rev ? (int64_t)rr.l_seq - 1 - k : k;
                const uint32_t byte = text[rr.seq + (src >> 1)];
                ws[b >> 2] |= bi_base((src & 1) ? (byte & 15u) : (byte >> 4), rev) << (8 * (b & 3));
                uint32_t ql = '!';
                if (d_qual && (rr.bits & BR_QUAL)) ql = ((uint32_t)text[rr.seq + (((int64_t)rr.l_seq + 1) >> 1) + src] + 33u) & 0xffu;
                wq[b >> 2] |= ql << (8 * (b & 3));
            }
            vs = make_uint4(ws[0], ws[1], ws[2], ws[3]);
            vq = make_uint4(wq[0], wq[1], wq[2], wq[3]);
        }
        *(uint4 *)(d_seq + p) = vs;
        if (d_qual) *(uint4 *)(d_qual + p) = vq;
    }
}

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_bam_last_device_ms(double *flatten_ms, double *walk_ms, double *decode_ms) {
    if (flatten_ms) *flatten_ms = tl_bam_ms[0];
    if (walk_ms) *walk_ms = tl_bam_ms[1];
    if (decode_ms) *decode_ms = tl_bam_ms[2];
}

extern "C" int32_t mpn_bam_flatten(int64_t n, const void *d_slots, const int64_t *slot_off, const int64_t *slot_len, const void *d_carry,
                                   int64_t carry_len, void *d_text, int64_t text_cap, int64_t *text_len) {
    tl_bam_ms[0] = 0;
    if (n < 0 || carry_len < 0 || (carry_len > 0 && !d_carry) || (n > 0 && (!slot_off || !slot_len)) || !text_len || text_cap < 0 ||
        ((uintptr_t)d_text & 15)) {
        set_error("mpn_bam_flatten: bad arguments");
        return -2;
    }
    std::vector<int64_t> dst, src, len;
    int64_t total = 0;
    if (carry_len > 0) { dst.push_back(0); src.push_back((int64_t)(uintptr_t)d_carry); len.push_back(carry_len); total = carry_len; }
    for (int64_t i = 0; i < n; ++i) {
        if (slot_off[i] < 0 || slot_len[i] < 0 || (slot_len[i] > 0 && !d_slots)) { set_error("mpn_bam_flatten: bad arguments"); return -2; }
        if (slot_len[i] == 0) continue;
        dst.push_back(total); src.push_back((int64_t)((uintptr_t)d_slots + (uintptr_t)slot_off[i])); len.push_back(slot_len[i]);
        total += slot_len[i];
    }
    *text_len = total;
    const int64_t out_bytes = (total + 15) & ~(int64_t)15;
    if (out_bytes > text_cap || (out_bytes > 0 && !d_text)) { set_error("mpn_bam_flatten: %lld bytes of text do not fit", (long long)out_bytes); return -2; }
    if (total == 0) return 0;
    {   // the carry must not overlap what is written
        const uintptr_t a = (uintptr_t)d_carry, b = (uintptr_t)d_text;
        if (carry_len > 0 && a < b + (uintptr_t)out_bytes && b < a + (uintptr_t)carry_len) { set_error("mpn_bam_flatten: the carry overlaps the text"); return -2; }
    }
    hipStream_t st = 0;
    DevBuf<int64_t> d_dst, d_src, d_len;
    DevTimer tm;
    const size_t S = dst.size();
    if (d_dst.upload(dst.data(), S, st) || d_src.upload(src.data(), S, st) || d_len.upload(len.data(), S, st) || tm.start(st)) return -1;
    hipLaunchKernelGGL(bam_flatten_kernel, dim3(grid_for(out_bytes)), dim3(G16_THREADS), 0, st, (const int64_t *)d_dst.p, (const int64_t *)d_src.p,
                       (const int64_t *)d_len.p, (int64_t)S, (uint8_t *)d_text, out_bytes);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));      // the segment arrays must outlive the kernel
    return tm.elapsed_ms(&tl_bam_ms[0]);
}

extern "C" int32_t mpn_bam_walk(const void *d_text, int64_t text_len, int64_t start, int32_t at_header, int32_t final, int64_t max_records,
                                mpn_bam_row *rows, int64_t *n_records, int64_t *next, int32_t *status) {
    tl_bam_ms[1] = 0;
    if (text_len < 0 || start < 0 || start > text_len || (text_len > 0 && !d_text) || max_records < 0 || max_records > 0x7fffffff ||
        (max_records > 0 && !rows) || !n_records || !next || !status) {
        set_error("mpn_bam_walk: bad arguments");
        return -2;
    }
    hipStream_t st = 0;
    DevBuf<mpn_bam_row> d_rows;
    DevBuf<int64_t> d_res;
    DevTimer tm;
    if (d_rows.alloc((size_t)max_records) || d_res.alloc(3) || tm.start(st)) return -1;
    hipLaunchKernelGGL(bam_walk_kernel, dim3(1), dim3(64), 0, st, (const uint8_t *)d_text, text_len, start, (int)(at_header != 0), (int)(final != 0),
                       max_records, d_rows.p, d_res.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    int64_t res[3] = {0, 0, 0};
    if (d_res.download(res, 3, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (res[0] < 0 || res[0] > max_records) { set_error("mpn_bam_walk: the kernel reported %lld records", (long long)res[0]); return -1; }
    if (d_rows.download(rows, (size_t)res[0], st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    *n_records = res[0]; *next = res[1]; *status = (int32_t)res[2];
    return tm.elapsed_ms(&tl_bam_ms[1]);
}

extern "C" int32_t mpn_bam_decode(const void *d_text, int64_t text_len, int64_t n, const mpn_bam_row *rows, const int64_t *out_off, void *d_seq,
                                  void *d_qual, char *name_pool, int64_t name_pool_cap) {
    tl_bam_ms[2] = 0;
    if (n < 0 || n > 0x7fffffff || text_len < 0 || (n > 0 && (!rows || !out_off || !d_text)) || !d_seq || name_pool_cap < 0 ||
        (name_pool_cap > 0 && !name_pool) || (((uintptr_t)d_seq | (uintptr_t)d_qual) & 15)) {
        set_error("mpn_bam_decode: bad arguments");
        return -2;
    }
    std::vector<int64_t> pool_off((size_t)n);
    int64_t total = 0, pool = 0;
    for (int64_t r = 0; r < n; ++r) {
        const mpn_bam_row &w = rows[r];
        if (w.off < 0 || w.off > text_len - BAMW_FIXED || w.l_seq < 0 || w.l_read_name < 1 || out_off[r] != total) {
            set_error("mpn_bam_decode: row %lld does not fit the text, or out_off is not the exclusive sum of l_seq", (long long)r);
            return -2;
        }
        total += w.l_seq;
        pool_off[(size_t)r] = pool;
        pool += w.l_read_name - 1;
    }
    if (pool > name_pool_cap) { set_error("mpn_bam_decode: the names need %lld bytes", (long long)pool); return -3; }
    const int64_t out_bytes = (total + 16 + 15) & ~(int64_t)15;
    hipStream_t st = 0;
    if (n == 0) {
        MPN_HIP_CHECK(hipMemsetAsync(d_seq, 0, (size_t)out_bytes, st));
        if (d_qual) MPN_HIP_CHECK(hipMemsetAsync(d_qual, 0, (size_t)out_bytes, st));
        MPN_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    // the CSR of records per chunk: chunk c is touched by records chunk_rec[c] .. chunk_rec[c + 1] (the last records that start at
    // or before its first byte and at or before the first byte of the next chunk)
    const int64_t n_chunks = (out_bytes + MPN_BAM_CHUNK - 1) / MPN_BAM_CHUNK;
    std::vector<int32_t> chunk_rec((size_t)n_chunks + 1);
    {
        int64_t j = 0;
        for (int64_t c = 0; c <= n_chunks; ++c) {
            while (j + 1 < n && out_off[j + 1] <= c * MPN_BAM_CHUNK) ++j;
            chunk_rec[(size_t)c] = (int32_t)j;
        }
    }
    DevBuf<mpn_bam_row> d_rows;
    DevBuf<int64_t> d_off, d_po;
    DevBuf<int32_t> d_cr, d_bad;
    DevBuf<BamRec> d_recs;
    DevBuf<uint8_t> d_pool;
    DevTimer tm;
    if (d_rows.upload(rows, (size_t)n, st) || d_off.upload(out_off, (size_t)n, st) || d_po.upload(pool_off.data(), (size_t)n, st) ||
        d_cr.upload(chunk_rec.data(), (size_t)n_chunks + 1, st) || d_recs.alloc((size_t)n) || d_pool.alloc((size_t)pool) || d_bad.alloc(1) ||
        d_bad.zero(st) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(bam_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_text, text_len,
                       (const mpn_bam_row *)d_rows.p, (const int64_t *)d_po.p, n, d_recs.p, d_pool.p, d_bad.p);
    hipLaunchKernelGGL(bam_decode_kernel, dim3(grid_for(out_bytes)), dim3(G16_THREADS), 0, st, (const uint8_t *)d_text, (const BamRec *)d_recs.p,
                       (const int64_t *)d_off.p, (const int32_t *)d_cr.p, out_bytes, (uint8_t *)d_seq, (uint8_t *)d_qual);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    int32_t bad = 0;
    if (d_bad.download(&bad, 1, st) || d_pool.download((uint8_t *)name_pool, (size_t)pool, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (tm.elapsed_ms(&tl_bam_ms[2])) return -1;
    if (bad) { set_error("mpn_bam_decode: a row's bases and qualities pass the end of the text"); return -2; }
    return 0;
}
