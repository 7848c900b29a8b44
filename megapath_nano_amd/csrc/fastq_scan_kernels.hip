// FASTQ text in HBM -> a table with a row per four-line record, and the bases and qualities of chosen rows in the layout of
// mapper.PackedReads.from_arrays, behind include/mpn_ingest.h (mpn_fastq_scan, mpn_fastq_gather).  The semantics are those of
// fastx.iter_fastx; the scan takes the longest prefix of records that are PLAIN (one line each for header, bases, '+' and
// qualities: the header says what that means), and what follows goes through the host path.
//
// In a plain record the bases and the qualities are each one contiguous span of the text, so nothing is moved here: the scan finds
// the spans, the gather copies them.  What a line is (header, bases, separator, qualities) cannot be told from its first byte -- a
// quality line may start with '@' -- but follows from its index modulo 4, and the index is the number of line feeds before it:
//   fq_count_kernel    per tile of MPN_FASTQ_TILE bytes: its line feeds.
//   fq_scan_kernel     one workgroup: the exclusive sums over the tiles.
//   fq_lines_kernel    per tile: the thread at a line feed stores where the next line starts (line_start[index]); every byte is
//                      checked against the kind of its line (a blank in the bases, a CR that no LF follows) and flags its LINE.
//                      A line longer than a tile -- the normal case for ONT reads -- needs nothing special: its bytes carry its index.
//   fq_rows_kernel     a thread per record: its four lines by their starts -> the row, and whether the record is plain.
//   fq_verdict_kernel  one workgroup: the first record that is not plain, hence n_records, consumed and the status.
// No atomics; the line flags are plain stores of one value.  Every read of the text is at an offset below text_len: line starts and
// ends come from line feeds that were seen in the text, or are text_len itself.
#include "gather16.h"

namespace mpn {

thread_local double tl_fastq_ms[2] = {0, 0};    // device time of the last calls on this thread: scan, gather

constexpr int FQ_THREADS = 256, FQ_PER = 16, FQ_TILE = FQ_THREADS * FQ_PER;
constexpr int FQ_SCAN_THREADS = 1024;
static_assert(FQ_TILE == MPN_FASTQ_TILE, "the tile the header promises");
static_assert(sizeof(mpn_fastq_row) == 32, "a row is two 16-byte stores");

__device__ __forceinline__ bool fq_is_blank(uint8_t c) { return c == ' ' || c == '\t' || c == '\v' || c == '\f'; }

struct FqBlock {
    alignas(16) uint8_t buf[FQ_TILE + 16];     // the tile and, at buf[len], the byte behind it (LF behind the end of the text)
    int wtot[4];
};

// the tile's bytes and the one behind them -> LDS; returns the number of bytes in the tile
__device__ __forceinline__ int fq_load(FqBlock &b, const uint8_t *__restrict__ text, int64_t text_len, int64_t tile) {
    const int64_t o = tile * FQ_TILE;
    const int len = (int)min((int64_t)FQ_TILE, text_len - o);
    const uint8_t *__restrict__ p = text + o;
    const int j0 = threadIdx.x * FQ_PER;
    if ((((uintptr_t)p) & 15) == 0 && j0 + FQ_PER <= len) {
        *(uint4 *)(b.buf + j0) = *(const uint4 *)(p + j0);
    } else {
        for (int j = j0; j < min(len, j0 + FQ_PER); ++j) b.buf[j] = p[j];
    }
    if (threadIdx.x == 0) b.buf[len] = o + len < text_len ? p[len] : (uint8_t)'\n';
    __syncthreads();
    return len;
}

// exclusive sum over the 256 threads; all: the sum of all of them
__device__ __forceinline__ int fq_excl_add(FqBlock &b, int v, int &all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_scan_add(v);
    if (lane == 63) b.wtot[wave] = incl;
    __syncthreads();
    int e = incl - v;
    all = 0;
    for (int k = 0; k < 4; ++k) { const int t = b.wtot[k]; if (k < wave) e += t; all += t; }
    return e;
}

__device__ __forceinline__ int fq_line_feeds(const FqBlock &b, int len) {
    const int j0 = threadIdx.x * FQ_PER, j1 = min(len, j0 + FQ_PER);
    int n = 0;
    for (int j = j0; j < j1; ++j) n += b.buf[j] == '\n';
    return n;
}

__global__ __launch_bounds__(FQ_THREADS) void fq_count_kernel(const uint8_t *__restrict__ text, int64_t text_len, int32_t *__restrict__ tile_lf) {
    __shared__ FqBlock b;
    const int len = fq_load(b, text, text_len, blockIdx.x);
    int all;
    fq_excl_add(b, fq_line_feeds(b, len), all);
    if (threadIdx.x == 0) tile_lf[blockIdx.x] = all;
}

// One workgroup.  lf_base[t]: the line feeds before tile t; lf_base[n_tiles]: all of them.
__global__ __launch_bounds__(FQ_SCAN_THREADS) void fq_scan_kernel(const int32_t *__restrict__ tile_lf, int64_t n_tiles, int64_t *__restrict__ lf_base) {
    __shared__ int64_t c_sum[FQ_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (n_tiles + FQ_SCAN_THREADS - 1) / FQ_SCAN_THREADS;
    const int64_t lo = min(n_tiles, tid * per), hi = min(n_tiles, lo + per);
    int64_t s = 0;
    for (int64_t t = lo; t < hi; ++t) s += tile_lf[t];
    c_sum[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int k = 0; k < FQ_SCAN_THREADS; ++k) { const int64_t v = c_sum[k]; c_sum[k] = run; run += v; }
        lf_base[n_tiles] = run;
    }
    __syncthreads();
    s = c_sum[tid];
    for (int64_t t = lo; t < hi; ++t) { lf_base[t] = s; s += tile_lf[t]; }
}

// line_start has n_lf + 2 entries: line i is text[line_start[i] .. line_start[i + 1] - 1), the byte at line_start[i + 1] - 1 being
// its line feed -- for the line behind the last line feed (index n_lf, possibly empty) the one imagined at text_len.
// line_bad has n_lf + 1 entries, zeroed by the caller.
__global__ __launch_bounds__(FQ_THREADS) void fq_lines_kernel(const uint8_t *__restrict__ text, int64_t text_len, const int64_t *__restrict__ lf_base,
                                                              int64_t n_lf, int64_t *__restrict__ line_start, uint8_t *__restrict__ line_bad) {
    __shared__ FqBlock b;
    const int64_t t = blockIdx.x;
    const int len = fq_load(b, text, text_len, t);
    int all;
    int64_t line = lf_base[t] + fq_excl_add(b, fq_line_feeds(b, len), all);
    if (t == 0 && threadIdx.x == 0) { line_start[0] = 0; line_start[n_lf + 1] = text_len + 1; }
    const int j0 = threadIdx.x * FQ_PER, j1 = min(len, j0 + FQ_PER);
    for (int j = j0; j < j1; ++j) {
        const uint8_t c = b.buf[j];
        const int kind = (int)(line & 3);
        // the text of the '+' line is ignored; a CR is part of a line end or the record is not plain
        const bool bad = kind != 2 && ((c == '\r' && b.buf[j + 1] != '\n') || (kind == 1 && fq_is_blank(c)));
        if (bad && line <= n_lf) line_bad[line] = 1;       // (every thread that stores stores the same value)
        if (c == '\n') {
            ++line;
            if (line <= n_lf) line_start[line] = t * FQ_TILE + j + 1;    // (the sums say that it is; the store checks it all the same)
        }
    }
}

// the lines that are whole: all that end in a line feed, and with `final_call` the text behind the last line feed, if there is any
__device__ __forceinline__ int64_t fq_whole_lines(const int64_t *__restrict__ line_start, int64_t n_lf, int64_t text_len, int final_call) {
    return n_lf + ((final_call && line_start[n_lf] < text_len) ? 1 : 0);
}

// a thread per candidate record r < n_cand = (n_lf + 1) / 4: lines 4r .. 4r + 3
__global__ __launch_bounds__(256) void fq_rows_kernel(const uint8_t *__restrict__ text, int64_t text_len, const int64_t *__restrict__ line_start,
                                                      const uint8_t *__restrict__ line_bad, int64_t n_lf, int final_call, int64_t n_cand,
                                                      mpn_fastq_row *__restrict__ rows, uint8_t *__restrict__ plain) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_cand) return;
    if (4 * r + 3 >= fq_whole_lines(line_start, n_lf, text_len, final_call)) { plain[r] = 0; return; }
    int64_t s[4], e[4];
    for (int i = 0; i < 4; ++i) {
        s[i] = line_start[4 * r + i];
        e[i] = line_start[4 * r + i + 1] - 1;          // its line feed, or text_len: s <= e <= text_len
        if (e[i] > s[i] && text[e[i] - 1] == '\r') --e[i];
    }
    const int64_t len = e[1] - s[1];
    bool ok = !line_bad[4 * r] && !line_bad[4 * r + 1] && !line_bad[4 * r + 3];
    ok = ok && e[0] > s[0] && text[s[0]] == '@' && e[2] > s[2] && text[s[2]] == '+' && e[3] - s[3] == len && len <= 0x7fffffff;
    if (ok && len > 0) { const uint8_t c = text[s[1]]; ok = c != '@' && c != '>' && c != '+'; }
    mpn_fastq_row row = {s[1], s[3], s[0], 0, 0};
    if (ok) {
        // the first word of the header line behind the '@' (bytes.split(): blank, TAB, LF, CR, VT and FF separate words)
        int64_t a = s[0] + 1;
        while (a < e[0] && (fq_is_blank(text[a]) || text[a] == '\r')) ++a;
        int64_t z = a;
        while (z < e[0] && !(fq_is_blank(text[z]) || text[z] == '\r')) ++z;
        row.name_off = a;
        row.len = (int32_t)len;
        row.name_len = (int32_t)min(z - a, (int64_t)0x7fffffff);
    }
    rows[r] = row;
    plain[r] = ok ? 1 : 0;
}

// One workgroup.  res[0] = n_records, res[1] = consumed, res[2] = status.
__global__ __launch_bounds__(FQ_SCAN_THREADS) void fq_verdict_kernel(const uint8_t *__restrict__ plain, int64_t n_cand, const int64_t *__restrict__ line_start,
                                                                     int64_t n_lf, int64_t text_len, int final_call, int64_t *__restrict__ res) {
    __shared__ int64_t c_first[FQ_SCAN_THREADS];
    int64_t first = n_cand;
    for (int64_t r = threadIdx.x; r < n_cand; r += FQ_SCAN_THREADS)
        if (!plain[r]) { first = r; break; }
    c_first[threadIdx.x] = first;
    __syncthreads();
    for (int step = FQ_SCAN_THREADS / 2; step > 0; step >>= 1) {
        if (threadIdx.x < step) c_first[threadIdx.x] = min(c_first[threadIdx.x], c_first[threadIdx.x + step]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t n = c_first[0];                                  // 4n <= n_lf + 1: an entry of line_start
        const int64_t consumed = min(line_start[4 * n], text_len);
        int64_t status = MPN_INFLATE_OK;
        if (consumed < text_len) {
            // text is left: a whole record that is not plain, or one the text ends in
            const bool whole = 4 * n + 3 < fq_whole_lines(line_start, n_lf, text_len, final_call);
            if (whole || final_call) status = MPN_FASTQ_UNSUPPORTED;
        }
        res[0] = n; res[1] = consumed; res[2] = status;
    }
}

// ---- gather --------------------------------------------------------------------------------------------------------------------
// As bam_flatten_kernel: a wave owns an aligned chunk of the OUTPUT, a lane 16 bytes of it; the rows that cover a chunk are found by
// binary search in out_off.  The same 16 places of d_seq and d_qual come from the same row, so one search serves both.
__global__ __launch_bounds__(G16_THREADS) void fq_gather_kernel(const uint8_t *__restrict__ text, const mpn_fastq_row *__restrict__ rows,
                                                                const int64_t *__restrict__ out_off, int64_t n, int64_t out_bytes,
                                                                uint8_t *__restrict__ d_seq, uint8_t *__restrict__ d_qual) {
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (out_bytes + G16_CHUNK - 1) / G16_CHUNK;
    for (int64_t c = (int64_t)blockIdx.x * G16_WAVES + (threadIdx.x >> 6); c < n_chunks; c += (int64_t)gridDim.x * G16_WAVES) {
        const int64_t c0 = c * G16_CHUNK;
        const int64_t c1 = (c0 + G16_CHUNK < out_bytes ? c0 + G16_CHUNK : out_bytes) - 1;
        // wave-uniform: the rows that can cover bytes of [c0, c1] (out_off[0] = 0, so jlo >= 0)
        const int64_t jlo = last_le(out_off, 0, n - 1, c0), jhi = last_le(out_off, jlo, n - 1, c1);
        const int64_t p = c0 + lane * 16;
        if (p >= out_bytes) continue;
        const int64_t j = last_le(out_off, jlo, jhi, p);
        const int64_t d = out_off[j];
        const mpn_fastq_row r = rows[j];
        uint4 vs = make_uint4(0, 0, 0, 0), vq = make_uint4(0, 0, 0, 0);
        if (p + 16 <= d + r.len) {
            vs = load16(text + r.seq_off + (p - d));
            if (d_qual) vq = load16(text + r.qual_off + (p - d));
        } else {
            // the end of a read, short reads, or the padding behind the last one: byte by byte
            uint32_t ws[4] = {0, 0, 0, 0}, wq[4] = {0, 0, 0, 0};
            int64_t jj = j;
#pragma unroll 1
            for (int b = 0; b < 16; ++b) {
                const int64_t q = p + b;
                jj = last_le(out_off, jj, jhi, q);
                const mpn_fastq_row rr = rows[jj];
                const int64_t k = q - out_off[jj];
                if (k >= rr.len) continue;
                ws[b >> 2] |= (uint32_t)text[rr.seq_off + k] << (8 * (b & 3));
                if (d_qual) wq[b >> 2] |= (uint32_t)text[rr.qual_off + k] << (8 * (b & 3));
            }
            vs = make_uint4(ws[0], ws[1], ws[2], ws[3]);
            vq = make_uint4(wq[0], wq[1], wq[2], wq[3]);
        }
        *(uint4 *)(d_seq + p) = vs;
        if (d_qual) *(uint4 *)(d_qual + p) = vq;
    }
}

// one thread per row: its name from the text into the pool
__global__ __launch_bounds__(256) void fq_names_kernel(const uint8_t *__restrict__ text, const mpn_fastq_row *__restrict__ rows,
                                                       const int64_t *__restrict__ pool_off, int64_t n, uint8_t *__restrict__ pool) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint8_t *__restrict__ p = text + rows[r].name_off;
    uint8_t *__restrict__ d = pool + pool_off[r];
    for (int k = 0; k < rows[r].name_len; ++k) d[k] = p[k];
}

}  // namespace mpn

using namespace mpn;

extern "C" int32_t mpn_fastq_tile(void) { return FQ_TILE; }

extern "C" void mpn_fastq_last_device_ms(double *scan_ms, double *gather_ms) {
    if (scan_ms) *scan_ms = tl_fastq_ms[0];
    if (gather_ms) *gather_ms = tl_fastq_ms[1];
}

extern "C" int32_t mpn_fastq_scan(const void *d_text, int64_t text_len, int32_t final, int64_t rec_cap, mpn_fastq_row *rows, int64_t *n_records,
                                  int64_t *consumed, int32_t *status) {
    tl_fastq_ms[0] = 0;
    if (text_len < 0 || (text_len > 0 && !d_text) || rec_cap < 0 || (rec_cap > 0 && !rows) || !n_records || !consumed || !status) {
        set_error("mpn_fastq_scan: bad arguments");
        return -2;
    }
    *n_records = 0; *consumed = 0; *status = MPN_INFLATE_OK;
    if (text_len == 0) return 0;
    const int64_t T = (text_len + FQ_TILE - 1) / FQ_TILE;
    if (T > 0x7fffffff) { set_error("mpn_fastq_scan: %lld tiles in one call", (long long)T); return -2; }
    const uint8_t *text = (const uint8_t *)d_text;
    const int final_call = final != 0;
    hipStream_t st = 0;
    DevBuf<int32_t> d_tile;
    DevBuf<int64_t> d_base, d_start, d_res;
    DevBuf<uint8_t> d_bad, d_plain;
    DevBuf<mpn_fastq_row> d_rows;
    DevTimer tm;
    if (d_tile.alloc((size_t)T) || d_base.alloc((size_t)T + 1) || d_res.alloc(3) || tm.start(st)) return -1;
    hipLaunchKernelGGL(fq_count_kernel, dim3((unsigned)T), dim3(FQ_THREADS), 0, st, text, text_len, d_tile.p);
    hipLaunchKernelGGL(fq_scan_kernel, dim3(1), dim3(FQ_SCAN_THREADS), 0, st, (const int32_t *)d_tile.p, T, d_base.p);
    MPN_HIP_CHECK(hipGetLastError());
    int64_t n_lf = 0;
    MPN_HIP_CHECK(hipMemcpyAsync(&n_lf, d_base.p + T, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (n_lf < 0 || n_lf > text_len) { set_error("mpn_fastq_scan: the kernel reported %lld line feeds", (long long)n_lf); return -1; }
    const int64_t n_cand = (n_lf + 1) / 4;
    if (d_start.alloc((size_t)n_lf + 2) || d_bad.alloc((size_t)n_lf + 1) || d_bad.zero(st) || d_rows.alloc((size_t)n_cand) || d_plain.alloc((size_t)n_cand))
        return -1;
    hipLaunchKernelGGL(fq_lines_kernel, dim3((unsigned)T), dim3(FQ_THREADS), 0, st, text, text_len, (const int64_t *)d_base.p, n_lf, d_start.p, d_bad.p);
    if (n_cand > 0)
        hipLaunchKernelGGL(fq_rows_kernel, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, st, text, text_len, (const int64_t *)d_start.p,
                           (const uint8_t *)d_bad.p, n_lf, final_call, n_cand, d_rows.p, d_plain.p);
    hipLaunchKernelGGL(fq_verdict_kernel, dim3(1), dim3(FQ_SCAN_THREADS), 0, st, (const uint8_t *)d_plain.p, n_cand, (const int64_t *)d_start.p, n_lf,
                       text_len, final_call, d_res.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    int64_t res[3] = {0, 0, 0};
    if (d_res.download(res, 3, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (tm.elapsed_ms(&tl_fastq_ms[0])) return -1;
    if (res[0] < 0 || res[0] > n_cand || res[1] < 0 || res[1] > text_len) {
        set_error("mpn_fastq_scan: the kernel reported %lld records and %lld bytes", (long long)res[0], (long long)res[1]);
        return -1;
    }
    *n_records = res[0]; *consumed = res[1]; *status = (int32_t)res[2];
    if (!rows && rec_cap == 0) return 0;       // the counting call
    if (res[0] > rec_cap) { set_error("mpn_fastq_scan: %lld records do not fit", (long long)res[0]); return -3; }
    if (d_rows.download(rows, (size_t)res[0], st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int32_t mpn_fastq_gather(const void *d_text, int64_t text_len, int64_t n, const mpn_fastq_row *rows, const int64_t *out_off, void *d_seq,
                                    void *d_qual, char *name_pool, int64_t name_pool_cap) {
    tl_fastq_ms[1] = 0;
    if (n < 0 || n > 0x7fffffff || text_len < 0 || (n > 0 && (!rows || !out_off || !d_text)) || !d_seq || name_pool_cap < 0 ||
        (name_pool_cap > 0 && !name_pool) || (((uintptr_t)d_seq | (uintptr_t)d_qual) & 15)) {
        set_error("mpn_fastq_gather: bad arguments");
        return -2;
    }
    std::vector<int64_t> pool_off((size_t)n);
    int64_t total = 0, pool = 0;
    for (int64_t r = 0; r < n; ++r) {
        const mpn_fastq_row &w = rows[r];
        if (w.len < 0 || w.name_len < 0 || w.seq_off < 0 || w.qual_off < 0 || w.name_off < 0 || w.seq_off > text_len - w.len ||
            w.qual_off > text_len - w.len || w.name_off > text_len - w.name_len || out_off[r] != total) {
            set_error("mpn_fastq_gather: row %lld does not lie in the text, or out_off is not the exclusive sum of len", (long long)r);
            return -2;
        }
        total += w.len;
        pool_off[(size_t)r] = pool;
        pool += w.name_len;
    }
    if (pool > name_pool_cap) { set_error("mpn_fastq_gather: the names need %lld bytes", (long long)pool); return -3; }
    const int64_t out_bytes = (total + 16 + 15) & ~(int64_t)15;
    hipStream_t st = 0;
    if (n == 0) {
        MPN_HIP_CHECK(hipMemsetAsync(d_seq, 0, (size_t)out_bytes, st));
        if (d_qual) MPN_HIP_CHECK(hipMemsetAsync(d_qual, 0, (size_t)out_bytes, st));
        MPN_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    DevBuf<mpn_fastq_row> d_rows;
    DevBuf<int64_t> d_off, d_po;
    DevBuf<uint8_t> d_pool;
    DevTimer tm;
    if (d_rows.upload(rows, (size_t)n, st) || d_off.upload(out_off, (size_t)n, st) || d_po.upload(pool_off.data(), (size_t)n, st) ||
        d_pool.alloc((size_t)pool) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(fq_gather_kernel, dim3(grid_for(out_bytes)), dim3(G16_THREADS), 0, st, (const uint8_t *)d_text, (const mpn_fastq_row *)d_rows.p,
                       (const int64_t *)d_off.p, n, out_bytes, (uint8_t *)d_seq, (uint8_t *)d_qual);
    if (pool > 0)
        hipLaunchKernelGGL(fq_names_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_text, (const mpn_fastq_row *)d_rows.p,
                           (const int64_t *)d_po.p, n, d_pool.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    if (d_pool.download((uint8_t *)name_pool, (size_t)pool, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));       // the uploaded arrays must outlive the kernels
    return tm.elapsed_ms(&tl_fastq_ms[1]);
}
