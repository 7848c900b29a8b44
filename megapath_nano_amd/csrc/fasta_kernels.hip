// FASTA text in HBM -> concatenated bases + record table, behind include/mpn_ingest.h (mpn_fasta_scan).  The semantics are those
// of fastx.iter_fastx on one file's bytes; what that function would treat differently from plain FASTA gets MPN_FASTA_UNSUPPORTED
// and goes through the host path.
//
// Whether a byte starts a line is local (the byte before it is LF, or it is the first of its stream), and so is the kind of a line
// (header: its first byte is '>').  What is not local is the kind of the line a tile BEGINS in, the number of sequence bytes
// before a tile and the number of records before it.  Three launches, no atomics, in the manner of the segmented scans of
// interval_kernels.hip:
//   fa_summary_kernel   per tile of 4096 bytes (tiles do not span streams): the bytes before the tile's first line start that
//                       are neither CR nor LF (sequence if the incoming line is a sequence line), the sequence bytes after it,
//                       the records that start in it, whether it holds a line start and the kind of its last line.
//   fa_scan_kernel      one workgroup: exclusive sums of sequence bytes and records over all tiles, and every tile's incoming
//                       kind (the summaries compose associatively: a line longer than a tile passes its kind on).
//   fa_scatter_kernel   per tile: every sequence byte to its place, every header to its row of the record table (the thread at
//                       the '>' walks the header line for the first word), and the reasons for UNSUPPORTED.
// The first tile of a stream starts with a line start, so nothing is carried from one stream into the next.
#include "mpn_common.h"
#include "../../include/mpn_ingest.h"

namespace mpn {

constexpr int FA_THREADS = 256, FA_PER = 16, FA_TILE = FA_THREADS * FA_PER;
constexpr int FA_SCAN_THREADS = 1024;
constexpr int FA_SEQ = 0, FA_HDR = 1, FA_INHERIT = 2;

struct FaTileSum { int32_t lead, rest, recs, flags; };      // flags: bit 0 = holds a line start, bit 1 = its last line is a header

__device__ __forceinline__ bool fa_is_blank(uint8_t c) { return c == ' ' || c == '\t' || c == '\v' || c == '\f'; }

// largest s with tile_first[s] <= t (streams without bytes have no tile)
__device__ __forceinline__ int fa_stream_of(const int64_t *__restrict__ tile_first, int n, int64_t t) {
    int lo = 0, hi = n;          // tile_first[lo] <= t < tile_first[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tile_first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

struct FaBlock {
    uint8_t buf[FA_TILE + 2];     // buf[0]: the byte before the tile (LF at a stream start), buf[1 + len]: the byte after it (LF at the end)
    int wtot[4][4];
};

// the tile's bytes and its two neighbours -> LDS; returns the number of bytes in the tile
__device__ __forceinline__ int fa_load(FaBlock &b, const uint8_t *__restrict__ text, int64_t s_begin, int64_t s_len, int64_t tile_in_stream) {
    const int64_t o = tile_in_stream * FA_TILE;
    const int len = (int)min((int64_t)FA_TILE, s_len - o);
    const uint8_t *__restrict__ p = text + s_begin + o;
    for (int k = threadIdx.x; k < len; k += FA_THREADS) b.buf[1 + k] = p[k];
    if (threadIdx.x == 0) {
        b.buf[0] = o > 0 ? p[-1] : (uint8_t)'\n';
        b.buf[1 + len] = o + len < s_len ? p[len] : (uint8_t)'\n';
    }
    __syncthreads();
    return len;
}

// exclusive max / sums over the 256 threads (slot: which wtot row; a kernel uses every row once, so one barrier per call is enough)
__device__ __forceinline__ int fa_excl_max(FaBlock &b, int slot, int v, int &all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_scan_max(v);
    if (lane == 63) b.wtot[slot][wave] = incl;
    __syncthreads();
    int e = wave_shr1(incl, 0);
    all = 0;
    for (int k = 0; k < 4; ++k) { const int t = b.wtot[slot][k]; if (k < wave) e = max(e, t); all = max(all, t); }
    return e;
}
__device__ __forceinline__ int fa_excl_add(FaBlock &b, int slot, int v, int &all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_scan_add(v);
    if (lane == 63) b.wtot[slot][wave] = incl;
    __syncthreads();
    int e = incl - v;
    all = 0;
    for (int k = 0; k < 4; ++k) { const int t = b.wtot[slot][k]; if (k < wave) e += t; all += t; }
    return e;
}

// a thread's 16 bytes: 1 + the place of the last line start among them, doubled, + 1 if that line is a header; 0 = none
__device__ __forceinline__ int fa_last_line_start(const FaBlock &b, int len) {
    const int j0 = threadIdx.x * FA_PER, j1 = min(len, j0 + FA_PER);
    int v = 0;
    for (int j = j0; j < j1; ++j) if (b.buf[j] == '\n') v = ((j + 1) << 1) | (b.buf[1 + j] == '>' ? 1 : 0);
    return v;
}

__global__ __launch_bounds__(FA_THREADS) void fa_summary_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ text_off,
                                                                const int64_t *__restrict__ text_len, const int64_t *__restrict__ tile_first, int n,
                                                                FaTileSum *__restrict__ sums) {
    __shared__ FaBlock b;
    const int64_t t = blockIdx.x;
    const int s = fa_stream_of(tile_first, n, t);
    const int len = fa_load(b, text, text_off[s], text_len[s], t - tile_first[s]);
    int last_all;
    const int e = fa_excl_max(b, 0, fa_last_line_start(b, len), last_all);
    int kind = e ? (e & 1) : FA_INHERIT;
    int lead = 0, rest = 0, recs = 0;
    const int j0 = threadIdx.x * FA_PER, j1 = min(len, j0 + FA_PER);
    for (int j = j0; j < j1; ++j) {
        const uint8_t c = b.buf[1 + j];
        if (b.buf[j] == '\n') { kind = c == '>' ? FA_HDR : FA_SEQ; recs += c == '>'; }
        const int body = c != '\n' && c != '\r';
        lead += kind == FA_INHERIT ? body : 0;
        rest += kind == FA_SEQ ? body : 0;
    }
    int lead_all, rest_all, recs_all;
    fa_excl_add(b, 1, lead, lead_all);
    fa_excl_add(b, 2, rest, rest_all);
    fa_excl_add(b, 3, recs, recs_all);
    if (threadIdx.x == 0) sums[t] = FaTileSum{lead_all, rest_all, recs_all, (last_all ? 1 : 0) | ((last_all & 1) << 1)};
}

// One workgroup.  seq_base / rec_base [t]: sequence bytes / records before tile t ([n_tiles]: all of them); kind_in[t]: the kind of
// the line tile t begins in.
__global__ __launch_bounds__(FA_SCAN_THREADS) void fa_scan_kernel(const FaTileSum *__restrict__ sums, int64_t n_tiles, int64_t *__restrict__ seq_base,
                                                                  int64_t *__restrict__ rec_base, uint8_t *__restrict__ kind_in) {
    __shared__ int64_t c_lead[FA_SCAN_THREADS], c_fixed[FA_SCAN_THREADS], c_recs[FA_SCAN_THREADS];
    __shared__ int c_kind[FA_SCAN_THREADS];      // FA_INHERIT: no line start in the chunk
    const int tid = threadIdx.x;
    const int64_t per = (n_tiles + FA_SCAN_THREADS - 1) / FA_SCAN_THREADS;
    const int64_t lo = min(n_tiles, tid * per), hi = min(n_tiles, lo + per);
    {
        int64_t lead = 0, fixed = 0, recs = 0;
        int kind = FA_INHERIT;
        for (int64_t t = lo; t < hi; ++t) {
            const FaTileSum u = sums[t];
            if (kind == FA_INHERIT) lead += u.lead; else if (kind == FA_SEQ) fixed += u.lead;
            fixed += u.rest;
            recs += u.recs;
            if (u.flags & 1) kind = (u.flags >> 1) & 1;
        }
        c_lead[tid] = lead; c_fixed[tid] = fixed; c_recs[tid] = recs; c_kind[tid] = kind;
    }
    __syncthreads();
    if (tid == 0) {
        int64_t seq = 0, recs = 0;
        int kind = FA_SEQ;       // (never used: the first tile starts with a line start)
        for (int k = 0; k < FA_SCAN_THREADS; ++k) {
            const int64_t add = (kind == FA_SEQ ? c_lead[k] : 0) + c_fixed[k], r = c_recs[k];
            const int out = c_kind[k] == FA_INHERIT ? kind : c_kind[k];
            c_fixed[k] = seq; c_recs[k] = recs; c_kind[k] = kind;
            seq += add; recs += r; kind = out;
        }
        seq_base[n_tiles] = seq;
        rec_base[n_tiles] = recs;
    }
    __syncthreads();
    int64_t seq = c_fixed[tid], recs = c_recs[tid];
    int kind = c_kind[tid];
    for (int64_t t = lo; t < hi; ++t) {
        const FaTileSum u = sums[t];
        seq_base[t] = seq; rec_base[t] = recs; kind_in[t] = (uint8_t)kind;
        seq += (kind == FA_SEQ ? u.lead : 0) + u.rest;
        recs += u.recs;
        if (u.flags & 1) kind = (u.flags >> 1) & 1;
    }
}

// d_seq == nullptr: the counting call, which wants the statuses only.  seq_end / rec_end: the sizes of d_seq and of the record
// table; the sums of fa_scan_kernel say that no index reaches them, the stores check it all the same.
__global__ __launch_bounds__(FA_THREADS) void fa_scatter_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ text_off,
                                                                const int64_t *__restrict__ text_len, const int64_t *__restrict__ tile_first, int n,
                                                                const int64_t *__restrict__ seq_base, const int64_t *__restrict__ rec_base,
                                                                const uint8_t *__restrict__ kind_in, uint8_t *__restrict__ d_seq,
                                                                int32_t *__restrict__ status, int32_t *__restrict__ rec_stream,
                                                                int64_t *__restrict__ rec_name_off, int32_t *__restrict__ rec_name_len,
                                                                int64_t *__restrict__ rec_seq_start, int64_t seq_end, int64_t rec_end) {
    __shared__ FaBlock b;
    const int64_t t = blockIdx.x;
    const int s = fa_stream_of(tile_first, n, t);
    const int64_t s_begin = text_off[s], s_len = text_len[s], tile_pos = (t - tile_first[s]) * FA_TILE;
    const int len = fa_load(b, text, s_begin, s_len, t - tile_first[s]);
    int unused;
    const int e = fa_excl_max(b, 0, fa_last_line_start(b, len), unused);
    const int kind0 = e ? (e & 1) : (int)kind_in[t];
    const int j0 = threadIdx.x * FA_PER, j1 = min(len, j0 + FA_PER);
    int kind = kind0, nseq = 0, nrec = 0;
    bool bad = false;
    for (int j = j0; j < j1; ++j) {
        const uint8_t c = b.buf[1 + j];
        if (b.buf[j] == '\n') { kind = c == '>' ? FA_HDR : FA_SEQ; nrec += c == '>'; bad |= c == '@' || c == '+'; }
        if (kind != FA_SEQ) continue;
        const uint8_t nx = b.buf[2 + j];
        bad |= fa_is_blank(c) || (c == '\r' && nx != '\n' && nx != '\r');
        nseq += c != '\n' && c != '\r';
    }
    int all;
    const int seq_excl = fa_excl_add(b, 1, nseq, all), rec_excl = fa_excl_add(b, 2, nrec, all);
    const int64_t seq0 = seq_base[t] + seq_excl, rec0 = rec_base[t] + rec_excl;
    kind = kind0;
    int iseq = 0, irec = 0;
    for (int j = j0; j < j1; ++j) {
        const uint8_t c = b.buf[1 + j];
        if (b.buf[j] == '\n') {
            kind = c == '>' ? FA_HDR : FA_SEQ;
            if (c == '>') {
                if (rec_stream && rec0 + irec < rec_end) {
                    // the first word of the header line (bytes.split(): blank, TAB, LF, CR, VT and FF separate words)
                    const uint8_t *__restrict__ p = text + s_begin;
                    int64_t a = tile_pos + j + 1;
                    while (a < s_len && (fa_is_blank(p[a]) || p[a] == '\r')) ++a;
                    int64_t z = a;
                    while (z < s_len && !(fa_is_blank(p[z]) || p[z] == '\r' || p[z] == '\n')) ++z;
                    const int64_t r = rec0 + irec;
                    rec_stream[r] = s;
                    rec_name_off[r] = s_begin + a;
                    rec_name_len[r] = (int32_t)min(z - a, (int64_t)0x7fffffff);
                    rec_seq_start[r] = seq0 + iseq;
                }
                ++irec;
            }
        }
        if (kind != FA_SEQ || c == '\n' || c == '\r') continue;
        bad |= rec0 + irec == rec_base[tile_first[s]];      // sequence before the stream's first header: iter_fastx raises on it
        if (d_seq && seq0 + iseq < seq_end) d_seq[seq0 + iseq] = c;
        ++iseq;
    }
    if (bad) status[s] = MPN_FASTA_UNSUPPORTED;     // (every thread that stores stores the same value)
}

// one thread per record: its name from the text into the pool
__global__ __launch_bounds__(256) void fa_names_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ name_off,
                                                       const int32_t *__restrict__ name_len, const int64_t *__restrict__ pool_off, int64_t n_rec,
                                                       uint8_t *__restrict__ pool) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    const uint8_t *__restrict__ p = text + name_off[r];
    uint8_t *__restrict__ d = pool + pool_off[r];
    for (int k = 0; k < name_len[r]; ++k) d[k] = p[k];
}

}  // namespace mpn

using namespace mpn;

extern "C" int32_t mpn_fasta_scan(int64_t n, const void *d_text, const int64_t *text_off, const int64_t *text_len, void *d_seq, int64_t seq_cap,
                                  int64_t *n_records, int64_t *n_bases, int32_t *status, int64_t rec_cap, int32_t *rec_stream,
                                  int64_t *rec_name_off, int32_t *rec_name_len, int64_t *rec_seq_len, char *name_pool, int64_t name_pool_cap) {
    tl_ingest_ms[1] = 0;
    const bool full = d_seq != nullptr || rec_cap > 0;
    if (n < 0 || n > 0x7fffffff || (n > 0 && (!text_off || !text_len || !n_records || !n_bases || !status)) || seq_cap < 0 || rec_cap < 0 ||
        name_pool_cap < 0 || (rec_cap > 0 && (!rec_stream || !rec_name_off || !rec_name_len || !rec_seq_len)) || (name_pool_cap > 0 && !name_pool)) {
        set_error("mpn_fasta_scan: bad arguments");
        return -2;
    }
    std::vector<int64_t> tile_first((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (text_len[i] < 0 || text_off[i] < 0 || (text_len[i] > 0 && !d_text)) { set_error("mpn_fasta_scan: bad arguments"); return -2; }
        tile_first[i + 1] = tile_first[i] + (text_len[i] + FA_TILE - 1) / FA_TILE;
        n_records[i] = 0; n_bases[i] = 0; status[i] = MPN_INFLATE_OK;
    }
    const int64_t T = tile_first[(size_t)n];
    if (T == 0) return 0;
    if (T > 0x7fffffff) { set_error("mpn_fasta_scan: %lld tiles in one call", (long long)T); return -2; }
    hipStream_t st = 0;
    DevBuf<int64_t> d_off, d_len, d_tf, d_sb, d_rb, d_rno, d_rss, d_po;
    DevBuf<FaTileSum> d_sums;
    DevBuf<uint8_t> d_kind, d_pool;
    DevBuf<int32_t> d_stat, d_rs, d_rnl;
    DevTimer tm;
    if (d_off.upload(text_off, (size_t)n, st) || d_len.upload(text_len, (size_t)n, st) || d_tf.upload(tile_first.data(), (size_t)n + 1, st) ||
        d_sums.alloc((size_t)T) || d_sb.alloc((size_t)T + 1) || d_rb.alloc((size_t)T + 1) || d_kind.alloc((size_t)T) || d_stat.alloc((size_t)n) ||
        d_stat.zero(st) || tm.start(st))
        return -1;
    const uint8_t *text = (const uint8_t *)d_text;
    hipLaunchKernelGGL(fa_summary_kernel, dim3((unsigned)T), dim3(FA_THREADS), 0, st, text, (const int64_t *)d_off.p, (const int64_t *)d_len.p,
                       (const int64_t *)d_tf.p, (int)n, d_sums.p);
    hipLaunchKernelGGL(fa_scan_kernel, dim3(1), dim3(FA_SCAN_THREADS), 0, st, (const FaTileSum *)d_sums.p, T, d_sb.p, d_rb.p, d_kind.p);
    MPN_HIP_CHECK(hipGetLastError());
    std::vector<int64_t> sb((size_t)T + 1), rb((size_t)T + 1);
    if (d_sb.download(sb.data(), (size_t)T + 1, st) || d_rb.download(rb.data(), (size_t)T + 1, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) {
        n_records[i] = rb[(size_t)tile_first[i + 1]] - rb[(size_t)tile_first[i]];
        n_bases[i] = sb[(size_t)tile_first[i + 1]] - sb[(size_t)tile_first[i]];
    }
    const int64_t R = rb[(size_t)T], B = sb[(size_t)T];
    if (full && (R > rec_cap || B > seq_cap)) { set_error("mpn_fasta_scan: %lld records and %lld bases do not fit", (long long)R, (long long)B); return -3; }
    if (full && (d_rs.alloc((size_t)R) || d_rno.alloc((size_t)R) || d_rnl.alloc((size_t)R) || d_rss.alloc((size_t)R))) return -1;
    hipLaunchKernelGGL(fa_scatter_kernel, dim3((unsigned)T), dim3(FA_THREADS), 0, st, text, (const int64_t *)d_off.p, (const int64_t *)d_len.p,
                       (const int64_t *)d_tf.p, (int)n, (const int64_t *)d_sb.p, (const int64_t *)d_rb.p, (const uint8_t *)d_kind.p,
                       full ? (uint8_t *)d_seq : nullptr, d_stat.p, full ? d_rs.p : nullptr, d_rno.p, d_rnl.p, d_rss.p, B, R);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    if (d_stat.download(status, (size_t)n, st)) return -1;
    std::vector<int64_t> starts((size_t)R);
    if (full && R > 0 &&
        (d_rs.download(rec_stream, (size_t)R, st) || d_rno.download(rec_name_off, (size_t)R, st) || d_rnl.download(rec_name_len, (size_t)R, st) ||
         d_rss.download(starts.data(), (size_t)R, st)))
        return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (tm.elapsed_ms(&tl_ingest_ms[1])) return -1;
    if (!full || R == 0) return 0;
    std::vector<int64_t> pool_off((size_t)R);
    int64_t pool = 0;
    for (int64_t r = 0; r < R; ++r) {
        rec_seq_len[r] = (r + 1 < R ? starts[(size_t)r + 1] : B) - starts[(size_t)r];
        pool_off[(size_t)r] = pool;
        pool += rec_name_len[r];
    }
    if (pool > name_pool_cap) { set_error("mpn_fasta_scan: the names need %lld bytes", (long long)pool); return -3; }
    if (pool == 0) return 0;
    if (d_po.upload(pool_off.data(), (size_t)R, st) || d_pool.alloc((size_t)pool)) return -1;
    hipLaunchKernelGGL(fa_names_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, text, (const int64_t *)d_rno.p, (const int32_t *)d_rnl.p,
                       (const int64_t *)d_po.p, R, d_pool.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (d_pool.download((uint8_t *)name_pool, (size_t)pool, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}
