// The read filter on the resident FASTQ text, behind include/mpn_ingest.h (mpn_fastq_heads, mpn_fastq_qsum_rows, mpn_fastq_emit):
// what `nanofastq` (fastq_filter.py) and `seqtk subseq` (fastx.subseq) need of a text mpn_fastq_scan has taken, without the bases
// and qualities existing on the host before they are output.
//   fqf_heads_kernel   a thread per row: the header line by the host filter's rule (id, separator, comment).
//   fqf_ids_kernel     a thread per row: the id into the pool that goes to the host.
//   fqf_qsum_kernel    a lane per read: the error sums of fastq_kernels.hip from the quality line where it lies, by 16-byte loads at
//                      any alignment; lane i takes row order[i] (a wave runs as long as its longest read, so the host MAY sort by
//                      length; it does not, profiles/r18_read_filter/README.md).
//   fqf_emit_kernel    the FASTQ text of the kept records: a chunked gather of gather16.h whose pieces are the seven segments of a
//                      record ('@', id, blank + comment, LF, bases, LF '+' LF, qualities, LF).
// Every read of the text is at an offset the host has checked against text_len, or lies between two such offsets.
#include "gather16.h"

namespace mpn {

thread_local double tl_fqf_ms[3] = {0, 0, 0};    // device time of the last calls on this thread: heads, sums, emit

static_assert(sizeof(mpn_fastq_head) == 16 && sizeof(mpn_fastq_pick) == 24, "the layouts the header promises");

__global__ __launch_bounds__(256) void fqf_heads_kernel(const uint8_t *__restrict__ text, const mpn_fastq_row *__restrict__ rows, int64_t n,
                                                        mpn_fastq_head *__restrict__ heads) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t lf = rows[r].seq_off - 1;         // the line feed of the header line (the host checked 1 <= lf < text_len)
    int64_t s = lf;                                 // back to the line's first byte: behind the previous line feed, or offset 0
    while (s > 0 && text[s - 1] != '\n') --s;
    const int64_t a = min(s + 1, lf);               // behind the '@'
    int64_t e = lf;
    if (e > a && text[e - 1] == '\r') --e;
    int64_t k = a;
    while (k < e && text[k] != ' ' && text[k] != '\t') ++k;
    mpn_fastq_head h;
    h.off = a;
    h.id_len = (int32_t)min(k - a, (int64_t)0x7fffffff);
    h.comment_len = k < e ? (int32_t)min(e - k - 1, (int64_t)0x7fffffff) : -1;
    heads[r] = h;
}

__global__ __launch_bounds__(256) void fqf_ids_kernel(const uint8_t *__restrict__ text, const mpn_fastq_head *__restrict__ heads,
                                                      const int64_t *__restrict__ pool_off, int64_t n, uint8_t *__restrict__ pool) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint8_t *__restrict__ p = text + heads[r].off;
    uint8_t *__restrict__ d = pool + pool_off[r];
    for (int k = 0; k < heads[r].id_len; ++k) d[k] = p[k];
}

// ---- sums ----------------------------------------------------------------------------------------------------------------------
// acc +/- tab[q - 33] for the cnt bytes at byte offset o of the aligned vectors v, one after the other; bad: a byte outside the table
// was met (its term is then some table entry: the caller discards the sums).  Whole steps of 16 bytes go through load16_at, whose
// two vectors both hold bytes of the step; the rest of less than 16 bytes is read byte by byte.
template <bool SUB>
__device__ __forceinline__ double fqf_terms(const uint4 *__restrict__ v, int64_t o, int32_t cnt, const double *tab, double acc, uint32_t &bad) {
    const uint4 *__restrict__ p = v + (o >> 4);
    const uint32_t sh = (uint32_t)(o & 15);
    int32_t k = 0;
    for (; k + 16 <= cnt; k += 16, ++p) {
        const uint4 w = load16_at(p, sh);
        const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const uint32_t c = ((x[b >> 2] >> (8 * (b & 3))) & 0xffu) - 33u;
            bad |= c > 127u;
            const double t = tab[c & 127u];
            acc = SUB ? acc - t : acc + t;
        }
    }
    const uint8_t *__restrict__ q = (const uint8_t *)v + o;
    for (; k < cnt; ++k) {
        const uint32_t c = (uint32_t)q[k] - 33u;
        bad |= c > 127u;
        const double t = tab[c & 127u];
        acc = SUB ? acc - t : acc + t;
    }
    return acc;
}

// text_al: the text's pointer rounded down to 16 bytes, shift: what was taken off it
__global__ __launch_bounds__(256) void fqf_qsum_kernel(const uint4 *__restrict__ text_al, int64_t shift, const mpn_fastq_row *__restrict__ rows,
                                                       const int32_t *__restrict__ order, int64_t n, int head_crop, int tail_crop, int min_len,
                                                       const double *__restrict__ table, double *__restrict__ total, double *__restrict__ cropped,
                                                       uint8_t *__restrict__ status) {
    __shared__ double tab[128];
    if (threadIdx.x < 128) tab[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = order ? order[i] : i;
    const int64_t o = rows[r].qual_off + shift;
    const int32_t l = rows[r].len;
    uint32_t bad = 0;
    const double t = fqf_terms<false>(text_al, o, l, tab, 0.0, bad);
    double c2 = t;
    const int64_t start = head_crop, end = (int64_t)l - tail_crop;
    if (!bad && end - start >= min_len) {          // (min_len >= 0: 0 <= start <= end <= l)
        c2 = fqf_terms<true>(text_al, o, (int32_t)start, tab, c2, bad);
        c2 = fqf_terms<true>(text_al, o + end, (int32_t)(l - end), tab, c2, bad);
    }
    total[r] = bad ? 0.0 : t;
    cropped[r] = bad ? 0.0 : c2;
    status[r] = bad ? 1 : 0;
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------
// A record of the output as its segments: the ends b1 .. b6 of id, comment, LF, bases, LF '+' LF and qualities, relative to the
// record's first byte (the '@' is byte 0, the last LF byte b6).
struct FqfRec {
    int64_t id_src, com_src, seq_src, qual_src;     // offsets into the text (id_src is not used with a serial)
    int64_t serial;                                 // 0: the header's id
    int32_t b1, b2, b3, b4, b5, b6;
};

__device__ __forceinline__ uint32_t fqf_byte(const FqfRec &w, int64_t k, const uint8_t *__restrict__ text, const uint8_t *__restrict__ prefix,
                                             int prefix_len) {
    if (k == 0) return '@';
    if (k < w.b1) {
        const int i = (int)k - 1;
        if (w.serial == 0) return text[w.id_src + i];
        if (i < prefix_len) return prefix[i];
        uint64_t s = (uint64_t)w.serial;
        for (int back = w.b1 - 1 - (int)k; back > 0; --back) s /= 10;     // the digit `back` places from the right
        return '0' + (uint32_t)(s % 10);
    }
    if (k < w.b2) return k == w.b1 ? (uint32_t)' ' : (uint32_t)text[w.com_src + (k - w.b1 - 1)];
    if (k < w.b3) return '\n';
    if (k < w.b4) return text[w.seq_src + (k - w.b3)];
    if (k < w.b5) return k == w.b4 + 1 ? '+' : '\n';
    if (k < w.b6) return text[w.qual_src + (k - w.b5)];
    return '\n';
}

// out_off has n + 1 entries (out_off[n] = total); out_bytes: total rounded up to 16
__global__ __launch_bounds__(G16_THREADS) void fqf_emit_kernel(const uint8_t *__restrict__ text, const FqfRec *__restrict__ recs,
                                                               const int64_t *__restrict__ out_off, int64_t n, int64_t total, int64_t out_bytes,
                                                               const uint8_t *__restrict__ prefix, int prefix_len, uint8_t *__restrict__ d_out) {
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (out_bytes + G16_CHUNK - 1) / G16_CHUNK;
    for (int64_t c = (int64_t)blockIdx.x * G16_WAVES + (threadIdx.x >> 6); c < n_chunks; c += (int64_t)gridDim.x * G16_WAVES) {
        const int64_t c0 = c * G16_CHUNK;
        const int64_t c1 = (c0 + G16_CHUNK < out_bytes ? c0 + G16_CHUNK : out_bytes) - 1;
        // wave-uniform: the records that can cover bytes of [c0, c1] (out_off[0] = 0, so jlo >= 0)
        const int64_t jlo = last_le(out_off, 0, n - 1, c0), jhi = last_le(out_off, jlo, n - 1, c1);
        const int64_t p = c0 + lane * 16;
        if (p >= out_bytes) continue;
        int64_t j = last_le(out_off, jlo, jhi, p);
        FqfRec w = recs[j];
        const int64_t k = p - out_off[j];
        uint4 v;
        if (k >= w.b3 && k + 16 <= w.b4) {
            v = load16(text + w.seq_src + (k - w.b3));
        } else if (k >= w.b5 && k + 16 <= w.b6) {
            v = load16(text + w.qual_src + (k - w.b5));
        } else {
            // a header, the seams of a record, short records, or the padding behind the last one: byte by byte
            uint32_t x[4] = {0, 0, 0, 0};
            int64_t end = out_off[j + 1];
#pragma unroll 1
            for (int b = 0; b < 16; ++b) {
                const int64_t q = p + b;
                if (q >= total) break;
                if (q >= end) {
                    j = last_le(out_off, j, jhi, q);
                    w = recs[j];
                    end = out_off[j + 1];
                }
                x[b >> 2] |= fqf_byte(w, q - out_off[j], text, prefix, prefix_len) << (8 * (b & 3));
            }
            v = make_uint4(x[0], x[1], x[2], x[3]);
        }
        *(uint4 *)(d_out + p) = v;
    }
}

static int fqf_rows_ok(const char *who, int64_t text_len, int64_t n, const mpn_fastq_row *rows, int64_t min_seq_off) {
    for (int64_t r = 0; r < n; ++r) {
        const mpn_fastq_row &w = rows[r];
        if (w.len < 0 || w.seq_off < min_seq_off || w.qual_off < 0 || w.seq_off > text_len - w.len || w.qual_off > text_len - w.len) {
            set_error("%s: row %lld does not lie in the text", who, (long long)r);
            return 0;
        }
    }
    return 1;
}

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_fastq_filter_last_device_ms(double *heads_ms, double *sums_ms, double *emit_ms) {
    if (heads_ms) *heads_ms = tl_fqf_ms[0];
    if (sums_ms) *sums_ms = tl_fqf_ms[1];
    if (emit_ms) *emit_ms = tl_fqf_ms[2];
}

extern "C" int32_t mpn_fastq_heads(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_row *rows, mpn_fastq_head *heads,
                                   char *name_pool, int64_t name_pool_cap) {
    tl_fqf_ms[0] = 0;
    if (n < 0 || n > 0x7fffffff || text_len < 0 || (n > 0 && (!rows || !heads || !d_text)) || name_pool_cap < 0 || (name_pool_cap > 0 && !name_pool)) {
        set_error("mpn_fastq_heads: bad arguments");
        return -2;
    }
    if (!fqf_rows_ok("mpn_fastq_heads", text_len, n, rows, 2)) return -2;
    if (n == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_fastq_row> d_rows;
    DevBuf<mpn_fastq_head> d_heads;
    DevTimer tm, tm2;
    if (d_rows.upload(rows, (size_t)n, st) || d_heads.alloc((size_t)n) || tm.start(st)) return -1;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(fqf_heads_kernel, dim3(grid), dim3(256), 0, st, (const uint8_t *)d_text, (const mpn_fastq_row *)d_rows.p, n, d_heads.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st) || d_heads.download(heads, (size_t)n, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (tm.elapsed_ms(&tl_fqf_ms[0])) return -1;
    std::vector<int64_t> pool_off((size_t)n);
    int64_t pool = 0;
    for (int64_t r = 0; r < n; ++r) {
        const mpn_fastq_head &h = heads[r];
        const int64_t com = h.comment_len < 0 ? 0 : 1 + (int64_t)h.comment_len;
        if (h.off < 1 || h.id_len < 0 || h.comment_len < -1 || h.off + h.id_len + com > rows[r].seq_off - 1) {
            set_error("mpn_fastq_heads: the kernel reported a header outside its line at row %lld", (long long)r);
            return -1;
        }
        pool_off[(size_t)r] = pool;
        pool += h.id_len;
    }
    if (!name_pool) return 0;
    if (pool > name_pool_cap) { set_error("mpn_fastq_heads: the ids need %lld bytes", (long long)pool); return -3; }
    if (pool == 0) return 0;
    DevBuf<int64_t> d_po;
    DevBuf<uint8_t> d_pool;
    if (d_po.upload(pool_off.data(), (size_t)n, st) || d_pool.alloc((size_t)pool) || tm2.start(st)) return -1;
    hipLaunchKernelGGL(fqf_ids_kernel, dim3(grid), dim3(256), 0, st, (const uint8_t *)d_text, (const mpn_fastq_head *)d_heads.p,
                       (const int64_t *)d_po.p, n, d_pool.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm2.stop(st) || d_pool.download((uint8_t *)name_pool, (size_t)pool, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    double ms = 0;
    if (tm2.elapsed_ms(&ms)) return -1;
    tl_fqf_ms[0] += ms;
    return 0;
}

extern "C" int32_t mpn_fastq_qsum_rows(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_row *rows, const int32_t *order,
                                       int32_t head_crop, int32_t tail_crop, int32_t min_len, const double *table, double *total, double *cropped,
                                       uint8_t *status) {
    tl_fqf_ms[1] = 0;
    if (n < 0 || n > 0x7fffffff || text_len < 0 || head_crop < 0 || tail_crop < 0 || min_len < 0 ||
        (n > 0 && (!rows || !d_text || !table || !total || !cropped || !status))) {
        set_error("mpn_fastq_qsum_rows: bad arguments");
        return -2;
    }
    if (!fqf_rows_ok("mpn_fastq_qsum_rows", text_len, n, rows, 0)) return -2;
    if (order) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int64_t i = 0; i < n; ++i) {
            if (order[i] < 0 || order[i] >= n || seen[(size_t)order[i]]) { set_error("mpn_fastq_qsum_rows: order is no permutation"); return -2; }
            seen[(size_t)order[i]] = 1;
        }
    }
    if (n == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_fastq_row> d_rows;
    DevBuf<int32_t> d_order;
    DevBuf<double> d_tab, d_total, d_crop;
    DevBuf<uint8_t> d_status;
    DevTimer tm;
    if (d_rows.upload(rows, (size_t)n, st) || (order && d_order.upload(order, (size_t)n, st)) || d_tab.upload(table, 128, st) ||
        d_total.alloc((size_t)n) || d_crop.alloc((size_t)n) || d_status.alloc((size_t)n) || tm.start(st))
        return -1;
    const uintptr_t shift = (uintptr_t)d_text & 15;
    hipLaunchKernelGGL(fqf_qsum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint4 *)((const uint8_t *)d_text - shift),
                       (int64_t)shift, (const mpn_fastq_row *)d_rows.p, order ? (const int32_t *)d_order.p : (const int32_t *)nullptr, n, head_crop,
                       tail_crop, min_len, (const double *)d_tab.p, d_total.p, d_crop.p, d_status.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st) || d_total.download(total, (size_t)n, st) || d_crop.download(cropped, (size_t)n, st) || d_status.download(status, (size_t)n, st))
        return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return tm.elapsed_ms(&tl_fqf_ms[1]);
}

extern "C" int32_t mpn_fastq_emit(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_row *rows, const mpn_fastq_head *heads,
                                  const mpn_fastq_pick *picks, const char *prefix, int32_t prefix_len, const int64_t *out_off, void *d_out,
                                  int64_t out_cap) {
    tl_fqf_ms[2] = 0;
    if (n < 0 || n > 0x7fffffff || text_len < 0 || prefix_len < 0 || (prefix_len > 0 && !prefix) || !out_off || out_cap < 0 ||
        (n > 0 && (!rows || !heads || !picks || !d_text || !d_out)) || ((uintptr_t)d_out & 15)) {
        set_error("mpn_fastq_emit: bad arguments");
        return -2;
    }
    if (!fqf_rows_ok("mpn_fastq_emit", text_len, n, rows, 0)) return -2;
    std::vector<FqfRec> recs((size_t)n);
    int64_t total = 0;
    for (int64_t r = 0; r < n; ++r) {
        const mpn_fastq_row &w = rows[r];
        const mpn_fastq_head &h = heads[r];
        const mpn_fastq_pick &k = picks[r];
        const int64_t com = h.comment_len < 0 ? 0 : h.comment_len;
        if (k.start < 0 || k.m < 0 || (int64_t)k.start + k.m > w.len || k.serial < 0 || h.off < 0 || h.id_len < 0 || h.comment_len < -1 ||
            h.off + h.id_len + (h.comment_len < 0 ? 0 : 1 + com) > text_len) {
            set_error("mpn_fastq_emit: the crop or the header of record %lld does not lie in its read or in the text", (long long)r);
            return -2;
        }
        int64_t id_len = h.id_len;
        if (k.serial > 0) {
            id_len = prefix_len;
            for (int64_t s = k.serial; s > 0; s /= 10) ++id_len;
        }
        const int64_t size = 1 + id_len + (k.with_comment ? 1 + com : 0) + 1 + k.m + 3 + k.m + 1;
        if (size > 0x7fffffff) { set_error("mpn_fastq_emit: record %lld is larger than 2^31 - 1 bytes", (long long)r); return -2; }
        if (out_off[r] != total || out_off[r + 1] != total + size) {
            set_error("mpn_fastq_emit: out_off is not the exclusive sum of the record sizes at record %lld", (long long)r);
            return -2;
        }
        FqfRec &f = recs[(size_t)r];
        f.id_src = h.off; f.com_src = h.off + h.id_len + 1; f.seq_src = w.seq_off + k.start; f.qual_src = w.qual_off + k.start;
        f.serial = k.serial;
        f.b1 = (int32_t)(1 + id_len);
        f.b2 = f.b1 + (k.with_comment ? (int32_t)(1 + com) : 0);
        f.b3 = f.b2 + 1; f.b4 = f.b3 + k.m; f.b5 = f.b4 + 3; f.b6 = f.b5 + k.m;
        total += size;
    }
    if (out_off[n] != total) { set_error("mpn_fastq_emit: out_off[n] is not the size of the output"); return -2; }
    const int64_t out_bytes = (total + 15) & ~(int64_t)15;
    if (out_bytes > out_cap) { set_error("mpn_fastq_emit: the output needs %lld bytes", (long long)out_bytes); return -2; }
    if (n == 0) return 0;
    hipStream_t st = 0;
    DevBuf<FqfRec> d_recs;
    DevBuf<int64_t> d_off;
    DevBuf<uint8_t> d_prefix;
    DevTimer tm;
    if (d_recs.upload(recs.data(), (size_t)n, st) || d_off.upload(out_off, (size_t)n + 1, st) ||
        d_prefix.upload((const uint8_t *)prefix, (size_t)prefix_len, st) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(fqf_emit_kernel, dim3(grid_for(out_bytes)), dim3(G16_THREADS), 0, st, (const uint8_t *)d_text, (const FqfRec *)d_recs.p,
                       (const int64_t *)d_off.p, n, total, out_bytes, (const uint8_t *)d_prefix.p, (int)prefix_len, (uint8_t *)d_out);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));       // the uploaded arrays must outlive the kernel
    return tm.elapsed_ms(&tl_fqf_ms[2]);
}
