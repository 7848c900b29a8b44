// Clair's input tensors from candidate sites, on a resident BAM text, behind include/mpn_tensor.h.  Semantics: Clair's
// preprocess/CreateTensor.py; the arithmetic shared with the host is csrc/tensor_core.h.
//
//   tens_records_kernel   a lane per record: tens_record (htslib's reference length, bases, qualities, a status).
//   tens_join_kernel      a wave per centre over its range of records: 64 records per step, a ballot of those that join, and a
//                         stable compaction behind the centre's offset of the pair list (count, scan on the host, scatter).
//   tens_flags_kernel     a wave per (deep centre, read) pair: the wave walks the read's operations 64 at a time
//                         (tens_wave_ops), the lane whose operation covers the centre decides (tens_flag_op).
//   tens_fill_kernel      a workgroup per tensor, its 1056 int32 in LDS, a wave per read at a time.  tens_wave_ops (tensor_wave.h) gives every
//                         lane the reference and query offset of its operation by two wave scans, skips the steps that end before
//                         the window and stops at the first that starts behind it; the lanes add what their operation says
//                         (tens_op: at most 33 positions, or the bases of an insertion) with LDS atomics.  The tile goes to HBM
//                         with plain vector stores.  Integer sums: the order does not show.
//   tens_emit_kernel      a block per line.  Lengths: the digits of the line's 1056 numbers, reduced over the block.  Writing:
//                         a block scan of the same widths places every number; thread 0 writes the name, the centre and the
//                         reference slice.
#include "mpn_common.h"
#include "tensor_core.h"
#include "tensor_wave.h"

namespace mpn {

using namespace mpn_tens;

static thread_local double tl_tens_ms[4] = {0, 0, 0, 0};     // join, flags, fill, emit

static_assert(sizeof(mpn_tensor_rec) == 16 && sizeof(mpn_tensor_read) == 16 && sizeof(mpn_tensor_job) == 24 && sizeof(mpn_tensor_line) == 24,
              "the layouts the Python layer reads");

constexpr int TENS_THREADS = 256, TENS_WAVES = TENS_THREADS / 64;
constexpr int EMIT_PER = 5;        // numbers of a line per thread: 256 x 5 >= 1056
static_assert(TENS_THREADS * EMIT_PER >= CELLS, "a block covers a line");

__global__ __launch_bounds__(256) void tens_records_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_bam_row *__restrict__ rows, int64_t n,
                                                           mpn_tensor_rec *__restrict__ recs) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    mpn_tensor_rec rec;
    tens_record(text, len, rows[r].off, &rec);       // (the host has checked off + 36 <= len)
    recs[r] = rec;
}

// ---- join ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TENS_THREADS) void tens_join_kernel(const int32_t *__restrict__ pos, const int64_t *__restrict__ span, int64_t n, int64_t m,
                                                                 const int32_t *__restrict__ c0, const int64_t *__restrict__ begin,
                                                                 const int64_t *__restrict__ end, int left_edge, const int64_t *__restrict__ pair_off,
                                                                 int32_t *__restrict__ pairs, int64_t pairs_cap, int64_t *__restrict__ counts) {
    const int64_t c = (int64_t)blockIdx.x * TENS_WAVES + (threadIdx.x >> 6);
    if (c >= m) return;                                      // (the whole wave)
    const int lane = threadIdx.x & 63;
    const int64_t b = begin[c], e = end[c] < n ? end[c] : n, centre = c0[c];
    const int64_t base = pairs ? pair_off[c] : 0;
    int64_t count = 0;
    for (int64_t r0 = b; r0 < e; r0 += 64) {
        const int64_t r = r0 + lane;
        const bool joins = r < e && tens_joins(pos[r], span[r], centre, left_edge);
        const unsigned long long vote = __ballot(joins);
        if (pairs && joins) {
            const int64_t at = base + count + __popcll(vote & ((1ull << lane) - 1ull));
            if (at < pairs_cap) pairs[at] = (int32_t)r;
        }
        count += __popcll(vote);
    }
    if (lane == 0) counts[c] = count;
}

// ---- centre flags --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TENS_THREADS) void tens_flags_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_tensor_read *__restrict__ reads,
                                                                  int64_t n_reads, const int32_t *__restrict__ pairs, int64_t n_pairs, int64_t n_f,
                                                                  const int64_t *__restrict__ pair, const int32_t *__restrict__ c0, int left_edge,
                                                                  uint8_t *__restrict__ flags, int32_t *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * TENS_WAVES + (threadIdx.x >> 6);
    if (i >= n_f) return;
    const int lane = threadIdx.x & 63;
    const int64_t pi = pair[i];
    if (pi < 0 || pi >= n_pairs) { if (lane == 0) { atomicMin(bad, 0); flags[i] = 0; } return; }
    const int64_t r = pairs[pi];
    if (r < 0 || r >= n_reads) { if (lane == 0) { atomicMin(bad, 0); flags[i] = 0; } return; }
    const mpn_tensor_read rd = reads[r];
    TensLayout L;
    if (!tens_layout(text, len, rd.off, &L)) { if (lane == 0) { atomicMin(bad, (int32_t)r); flags[i] = 0; } return; }
    const TensWin W{(int64_t)c0[i], tens_join_pos(rd.pos, c0[i], left_edge), nullptr, 0, 0};
    int mine = 0;
    const bool good = tens_wave_ops(text, L, rd.pos, W.c0, W.c0, lane, [&](uint32_t op, int64_t n, int64_t r0, int64_t q0) {
        const int f = tens_flag_op(text, L, op, n, r0, q0, W);
        if (f) mine = f;
    });
    const unsigned long long high = __ballot(mine > 0), none = __ballot(mine < 0);
    if (lane == 0) {
        if (!good || none) atomicMin(bad, (int32_t)r);
        flags[i] = high ? 1 : 0;
    }
}

// ---- fill ----------------------------------------------------------------------------------------------------------------------
struct TensLdsAdd {
    int32_t *tile;
    __device__ __forceinline__ void operator()(int cell) { atomicAdd(&tile[cell], 1); }
};

__global__ __launch_bounds__(TENS_THREADS) void tens_fill_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_tensor_read *__restrict__ reads,
                                                                 int64_t n_reads, const int32_t *__restrict__ pairs, int64_t n_pairs,
                                                                 const int64_t *__restrict__ sel, int64_t n_sel, const mpn_tensor_job *__restrict__ jobs,
                                                                 int left_edge, const uint8_t *__restrict__ ref, int64_t ref_start, int64_t ref_len,
                                                                 int32_t *__restrict__ tensors, int32_t *__restrict__ depth, int32_t *__restrict__ bad) {
    __shared__ int32_t s_tile[CELLS];
    const mpn_tensor_job job = jobs[blockIdx.x];
    for (int i = threadIdx.x; i < CELLS; i += TENS_THREADS) s_tile[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    TensLdsAdd add{s_tile};
    for (int i = threadIdx.x >> 6; i < job.n; i += TENS_WAVES) {
        int64_t pi = job.begin + i;
        if (job.via_sel) {
            if (pi < 0 || pi >= n_sel) { if (lane == 0) atomicMin(bad, 0); continue; }
            pi = sel[pi];
        }
        if (pi < 0 || pi >= n_pairs) { if (lane == 0) atomicMin(bad, 0); continue; }
        const int64_t r = pairs[pi];
        if (r < 0 || r >= n_reads) { if (lane == 0) atomicMin(bad, 0); continue; }
        const mpn_tensor_read rd = reads[r];
        TensLayout L;
        if (!tens_layout(text, len, rd.off, &L)) { if (lane == 0) atomicMin(bad, (int32_t)r); continue; }
        const TensWin W{(int64_t)job.c0, tens_join_pos(rd.pos, job.c0, left_edge), ref, ref_start, ref_len};
        const int strand = rd.reverse ? 4 : 0;
        int wrong = 0;
        const bool good = tens_wave_ops(text, L, rd.pos, W.c0 - FLANK, W.c0 + FLANK, lane, [&](uint32_t op, int64_t n, int64_t r0, int64_t q0) {
            wrong |= tens_op(text, L, op, n, r0, q0, strand, W, add);
        });
        if (!good || wrong) atomicMin(bad, (int32_t)r);
    }
    __syncthreads();
    int32_t *__restrict__ out = tensors + (int64_t)blockIdx.x * CELLS;
    for (int i = threadIdx.x; i < CELLS; i += TENS_THREADS) out[i] = s_tile[i];
    if (threadIdx.x == 0) {
        int32_t d = 0;
        for (int row = 0; row < ROWS; ++row) d += s_tile[(FLANK * ROWS + row) * CHANNELS];
        depth[blockIdx.x] = d;
    }
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------
// the sum of v over the block behind this thread (exclusive), and the block's total
__device__ __forceinline__ int tens_block_scan(int v, int *s_wave, int *total) {
    const int incl = wave_scan_add(v);
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < TENS_WAVES; ++k) {
        if (k < (int)(threadIdx.x >> 6)) before += s_wave[k];
        all += s_wave[k];
    }
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(TENS_THREADS) void tens_emit_kernel(const int32_t *__restrict__ tensors, const mpn_tensor_line *__restrict__ lines,
                                                                 const uint8_t *__restrict__ ref, const uint8_t *__restrict__ name, int name_len,
                                                                 int64_t *__restrict__ line_len, const int64_t *__restrict__ line_off,
                                                                 uint8_t *__restrict__ out, int64_t out_cap) {
    __shared__ int s_wave[TENS_WAVES];
    const mpn_tensor_line line = lines[blockIdx.x];
    const int32_t *__restrict__ t = tensors + line.tensor * CELLS;
    const int i0 = threadIdx.x * EMIT_PER;
    uint32_t v[EMIT_PER];
    int width = 0;
#pragma unroll
    for (int k = 0; k < EMIT_PER; ++k) {
        v[k] = i0 + k < CELLS ? (uint32_t)t[i0 + k] : 0u;
        if (i0 + k < CELLS) width += 1 + tens_digits(v[k]);          // a blank and the number
    }
    int total = 0;
    const int before = tens_block_scan(width, s_wave, &total);
    const int head = name_len + 1 + tens_digits((uint32_t)line.centre) + 1 + line.ref_n;
    if (!out) {
        if (threadIdx.x == 0) line_len[blockIdx.x] = (int64_t)head + total + 1;
        return;
    }
    const int64_t at0 = line_off[blockIdx.x];
    if (at0 < 0 || at0 + head + total + 1 > out_cap) return;          // (the host has refused such a call)
    if (threadIdx.x == 0) {
        int64_t at = at0;
        for (int k = 0; k < name_len; ++k) out[at++] = name[k];
        out[at++] = ' ';
        at += tens_put(out, at, out_cap, (uint32_t)line.centre);
        out[at++] = ' ';
        for (int k = 0; k < line.ref_n; ++k) out[at++] = ref[line.ref_off + k];
        out[at0 + head + total] = '\n';
    }
    int64_t at = at0 + head + before;
#pragma unroll
    for (int k = 0; k < EMIT_PER; ++k)
        if (i0 + k < CELLS) {
            out[at++] = ' ';
            at += tens_put(out, at, out_cap, v[k]);
        }
}

static int tens_time(DevTimer &tm, hipStream_t st, double *ms) {
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return tm.elapsed_ms(ms);
}

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_tensor_last_device_ms(double *join_ms, double *flags_ms, double *fill_ms, double *emit_ms) {
    if (join_ms) *join_ms = tl_tens_ms[0];
    if (flags_ms) *flags_ms = tl_tens_ms[1];
    if (fill_ms) *fill_ms = tl_tens_ms[2];
    if (emit_ms) *emit_ms = tl_tens_ms[3];
}

static bool tens_reads_inside(const mpn_tensor_read *reads, int64_t n, int64_t text_len) {
    for (int64_t r = 0; r < n; ++r)
        if (reads[r].off < 0 || reads[r].off > text_len - mpn_bamw::BAMW_FIXED) return false;
    return true;
}

extern "C" int32_t mpn_tensor_records(const void *d_text, int64_t text_len, int64_t n, const mpn_bam_row *rows, mpn_tensor_rec *recs) {
    if (n < 0 || n > 0x7fffffff || text_len < 0 || (n > 0 && (!rows || !recs || !d_text))) {
        set_error("mpn_tensor_records: bad arguments");
        return -2;
    }
    for (int64_t r = 0; r < n; ++r)
        if (rows[r].off < 0 || rows[r].off > text_len - mpn_bamw::BAMW_FIXED) {
            set_error("mpn_tensor_records: row %lld does not lie inside the text", (long long)r);
            return -2;
        }
    if (n == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_bam_row> d_rows;
    DevBuf<mpn_tensor_rec> d_recs;
    if (d_rows.upload(rows, (size_t)n, st) || d_recs.alloc((size_t)n)) return -1;
    hipLaunchKernelGGL(tens_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_text, text_len,
                       (const mpn_bam_row *)d_rows.p, n, d_recs.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (d_recs.download(recs, (size_t)n, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int32_t mpn_tensor_join(int64_t n, const int32_t *pos, const int64_t *span, int64_t m, const int32_t *c0, const int64_t *begin,
                                   const int64_t *end, int32_t left_edge, int64_t *counts, const int64_t *pair_off, void *d_pairs, int64_t pairs_cap) {
    tl_tens_ms[0] = 0;
    if (n < 0 || n > 0x7ffffff0 || m < 0 || m > 0x7ffffff0 || (n > 0 && (!pos || !span)) || (m > 0 && (!c0 || !begin || !end || !counts)) ||
        (d_pairs && (!pair_off || pairs_cap < 0))) {
        set_error("mpn_tensor_join: bad arguments");
        return -2;
    }
    for (int64_t c = 0; c < m; ++c)
        if (begin[c] < 0 || end[c] < begin[c] || end[c] > n || (c > 0 && c0[c] <= c0[c - 1]) || (d_pairs && (pair_off[c] < 0 || pair_off[c] > pairs_cap))) {
            set_error("mpn_tensor_join: centre %lld: its range does not lie inside the records, or the centres are not ascending", (long long)c);
            return -2;
        }
    if (m == 0) return 0;
    hipStream_t st = 0;
    DevBuf<int32_t> d_pos, d_c0;
    DevBuf<int64_t> d_span, d_begin, d_end, d_counts, d_off;
    DevTimer tm;
    if (d_pos.upload(pos, (size_t)n, st) || d_span.upload(span, (size_t)n, st) || d_c0.upload(c0, (size_t)m, st) || d_begin.upload(begin, (size_t)m, st) ||
        d_end.upload(end, (size_t)m, st) || d_counts.alloc((size_t)m) || (d_pairs ? d_off.upload(pair_off, (size_t)m, st) : 0) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(tens_join_kernel, dim3((unsigned)((m + TENS_WAVES - 1) / TENS_WAVES)), dim3(TENS_THREADS), 0, st, (const int32_t *)d_pos.p,
                       (const int64_t *)d_span.p, n, m, (const int32_t *)d_c0.p, (const int64_t *)d_begin.p, (const int64_t *)d_end.p, (int)left_edge,
                       (const int64_t *)(d_pairs ? d_off.p : nullptr), (int32_t *)d_pairs, pairs_cap, d_counts.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st) || d_counts.download(counts, (size_t)m, st)) return -1;
    return tens_time(tm, st, &tl_tens_ms[0]);
}

extern "C" int32_t mpn_tensor_centre_flags(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_tensor_read *reads, const void *d_pairs,
                                           int64_t n_pairs, int64_t n_f, const int64_t *pair, const int32_t *c0, int32_t left_edge, uint8_t *flags,
                                           int64_t *bad_read) {
    tl_tens_ms[1] = 0;
    if (n_reads < 0 || n_reads > 0x7ffffff0 || n_pairs < 0 || n_f < 0 || n_f > 0x7ffffff0 || text_len < 0 || !bad_read ||
        (n_f > 0 && (!d_text || !reads || !d_pairs || !pair || !c0 || !flags)) || !tens_reads_inside(reads, n_reads, text_len)) {
        set_error("mpn_tensor_centre_flags: bad arguments, or a read does not lie inside the text");
        return -2;
    }
    *bad_read = -1;
    if (n_f == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_tensor_read> d_reads;
    DevBuf<int64_t> d_pair;
    DevBuf<int32_t> d_c0, d_bad;
    DevBuf<uint8_t> d_flags;
    DevTimer tm;
    const int32_t none = 0x7fffffff;
    if (d_reads.upload(reads, (size_t)n_reads, st) || d_pair.upload(pair, (size_t)n_f, st) || d_c0.upload(c0, (size_t)n_f, st) ||
        d_flags.alloc((size_t)n_f) || d_bad.upload(&none, 1, st) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(tens_flags_kernel, dim3((unsigned)((n_f + TENS_WAVES - 1) / TENS_WAVES)), dim3(TENS_THREADS), 0, st, (const uint8_t *)d_text,
                       text_len, (const mpn_tensor_read *)d_reads.p, n_reads, (const int32_t *)d_pairs, n_pairs, n_f, (const int64_t *)d_pair.p,
                       (const int32_t *)d_c0.p, (int)left_edge, d_flags.p, d_bad.p);
    MPN_HIP_CHECK(hipGetLastError());
    int32_t bad = none;
    if (tm.stop(st) || d_flags.download(flags, (size_t)n_f, st) || d_bad.download(&bad, 1, st)) return -1;
    if (tens_time(tm, st, &tl_tens_ms[1])) return -1;
    if (bad != none) *bad_read = bad;
    return 0;
}

extern "C" int32_t mpn_tensor_fill(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_tensor_read *reads, const void *d_pairs,
                                   int64_t n_pairs, int64_t n_sel, const int64_t *sel, int64_t n_jobs, const mpn_tensor_job *jobs, int32_t left_edge,
                                   const void *d_ref, int64_t ref_start, int64_t ref_len, void *d_tensors, int32_t *depth, int64_t *bad_read) {
    tl_tens_ms[2] = 0;
    if (n_reads < 0 || n_reads > 0x7ffffff0 || n_pairs < 0 || n_sel < 0 || (n_sel > 0 && !sel) || n_jobs < 0 || n_jobs > 0x7ffffff0 || text_len < 0 ||
        ref_len < 0 || (ref_len > 0 && !d_ref) || !bad_read || (n_jobs > 0 && (!d_text || !reads || !d_pairs || !jobs || !d_tensors || !depth)) ||
        !tens_reads_inside(reads, n_reads, text_len)) {
        set_error("mpn_tensor_fill: bad arguments, or a read does not lie inside the text");
        return -2;
    }
    for (int64_t j = 0; j < n_jobs; ++j) {
        const mpn_tensor_job &b = jobs[j];
        if (b.n < 0 || b.n > MPN_TENSOR_DEPTH || b.begin < 0 || b.begin + b.n > (b.via_sel ? n_sel : n_pairs)) {
            set_error("mpn_tensor_fill: tensor %lld: its reads do not lie inside the list, or are more than %d", (long long)j, MPN_TENSOR_DEPTH);
            return -2;
        }
    }
    *bad_read = -1;
    if (n_jobs == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_tensor_read> d_reads;
    DevBuf<int64_t> d_sel;
    DevBuf<mpn_tensor_job> d_jobs;
    DevBuf<int32_t> d_depth, d_bad;
    DevTimer tm;
    const int32_t none = 0x7fffffff;
    if (d_reads.upload(reads, (size_t)n_reads, st) || d_sel.upload(sel, (size_t)n_sel, st) || d_jobs.upload(jobs, (size_t)n_jobs, st) ||
        d_depth.alloc((size_t)n_jobs) || d_bad.upload(&none, 1, st) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(tens_fill_kernel, dim3((unsigned)n_jobs), dim3(TENS_THREADS), 0, st, (const uint8_t *)d_text, text_len,
                       (const mpn_tensor_read *)d_reads.p, n_reads, (const int32_t *)d_pairs, n_pairs, (const int64_t *)d_sel.p, n_sel,
                       (const mpn_tensor_job *)d_jobs.p, (int)left_edge, (const uint8_t *)d_ref, ref_start, ref_len, (int32_t *)d_tensors, d_depth.p,
                       d_bad.p);
    MPN_HIP_CHECK(hipGetLastError());
    int32_t bad = none;
    if (tm.stop(st) || d_depth.download(depth, (size_t)n_jobs, st) || d_bad.download(&bad, 1, st)) return -1;
    if (tens_time(tm, st, &tl_tens_ms[2])) return -1;
    if (bad != none) *bad_read = bad;
    return 0;
}

extern "C" int32_t mpn_tensor_emit(const void *d_tensors, int64_t n_tensors, int64_t n_lines, const mpn_tensor_line *lines, const void *d_ref,
                                   int64_t ref_len, const char *name, int32_t name_len, int64_t *line_len, const int64_t *line_off, void *d_out,
                                   int64_t out_cap) {
    tl_tens_ms[3] = 0;
    if (n_tensors < 0 || n_lines < 0 || n_lines > 0x7ffffff0 || ref_len < 0 || name_len < 0 || name_len > 4096 || (name_len > 0 && !name) ||
        (n_lines > 0 && (!d_tensors || !lines || !line_len)) || (d_out && (!line_off || out_cap < 0))) {
        set_error("mpn_tensor_emit: bad arguments");
        return -2;
    }
    for (int64_t i = 0; i < n_lines; ++i) {
        const mpn_tensor_line &l = lines[i];
        if (l.tensor < 0 || l.tensor >= n_tensors || l.centre < 0 || l.ref_n < 0 || l.ref_n > MPN_TENSOR_POSITIONS || l.ref_off < 0 ||
            l.ref_off + l.ref_n > ref_len || (l.ref_n > 0 && !d_ref)) {
            set_error("mpn_tensor_emit: line %lld: its tensor or its reference slice does not exist", (long long)i);
            return -2;
        }
        if (d_out && (line_off[i] < 0 || line_len[i] < 0 || line_off[i] + line_len[i] > out_cap)) {
            set_error("mpn_tensor_emit: line %lld does not fit the output", (long long)i);
            return -3;
        }
    }
    if (n_lines == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_tensor_line> d_lines;
    DevBuf<uint8_t> d_name;
    DevBuf<int64_t> d_len, d_off;
    DevTimer tm;
    if (d_lines.upload(lines, (size_t)n_lines, st) || d_name.upload((const uint8_t *)name, (size_t)name_len, st) || d_len.alloc((size_t)n_lines) ||
        (d_out ? d_off.upload(line_off, (size_t)n_lines, st) : 0) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(tens_emit_kernel, dim3((unsigned)n_lines), dim3(TENS_THREADS), 0, st, (const int32_t *)d_tensors, (const mpn_tensor_line *)d_lines.p,
                       (const uint8_t *)d_ref, (const uint8_t *)d_name.p, (int)name_len, d_len.p, (const int64_t *)(d_out ? d_off.p : nullptr),
                       (uint8_t *)d_out, out_cap);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st) || (d_out ? 0 : d_len.download(line_len, (size_t)n_lines, st))) return -1;
    return tens_time(tm, st, &tl_tens_ms[3]);
}
