// The device side of include/mpn_read_realign.h: realign_illumina_reads.py's per-record fields, its pileup[...]["X"] counter and its
// find_max_overlap_index, on a BAM text that is resident.  The arithmetic shared with the host is csrc/read_realign_core.h.
//
//   rr_records_kernel   a lane per record: rr_record (fixed fields, the CIGAR sums, a scan of the bases for `=`, the aux walk).
//   rr_support_kernel   a workgroup per job.  A job is one epoch's row of 5041 positions and a slice of the records that can reach
//                       it (a contiguous range of the sorted takes, bisected on the host).  The row is in LDS (20 KiB).  A wave
//                       takes one record at a time with the shared CIGAR walk (tensor_wave.h, N not moving the reference): 64
//                       operations a step.  The bases of an M or X clipped to the row are taken by the whole wave when they are
//                       32 or more, by the operation's own lane otherwise.  I, S and D whose range meets the row and whose
//                       region and base-before tests hold are taken one after the other by the whole wave: the qualities of an
//                       I or S are tested 64 a step, every lane keeping its own flag across the steps and one ballot at the
//                       end, then the lanes add the clipped range.  All adds are LDS atomics; a row with one job is stored
//                       plainly, the jobs of a split row add with atomicAdd.  Integer sums: the order does not show.
//   rr_assign_kernel    a lane per (split, read): rr_assign_one, the window's number to `assign`, one atomic add to its count.
//   rr_compact_kernel   a workgroup per window that has reads (the host sums the counts into offsets between the two launches): it
//                       walks the reads of its split in order, 256 at a time, and writes those that are its own behind a ballot /
//                       prefix-count rank.
#include "mpn_common.h"
#include "read_realign_core.h"
#include "tensor_wave.h"

namespace mpn {

using namespace mpn_rr;

static thread_local double tl_rr_ms[3] = {0, 0, 0};       // device time of the last calls on this thread: records, support, assign

static_assert(sizeof(mpn_rr_rec) == 64 && sizeof(mpn_rr_take) == 24, "the layouts the Python layer reads");

constexpr int RR_THREADS = 256, RR_WAVES = RR_THREADS / 64;
constexpr int RR_WIDE = 32;            // clipped bases of one operation from which the whole wave takes them

struct RrJob { int32_t epoch, begin, end, plain; };

__global__ __launch_bounds__(256) void rr_records_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_bam_row *__restrict__ rows, int64_t n,
                                                         mpn_rr_rec *__restrict__ recs) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    mpn_rr_rec rec;
    rr_record(text, len, rows[r].off, &rec);         // (the host has checked off + 36 <= len)
    recs[r] = rec;
}

__device__ __forceinline__ void rr_flag_bad(int32_t *bad, int64_t r) { atomicMin(bad, (int32_t)r); }

__global__ __launch_bounds__(RR_THREADS) void rr_support_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_rr_take *__restrict__ takes,
                                                                const RrJob *__restrict__ jobs, const int32_t *__restrict__ row_lo,
                                                                const uint8_t *__restrict__ contig, int64_t contig_len, int32_t *__restrict__ rows,
                                                                int32_t *__restrict__ bad) {
    __shared__ int32_t s_row[RR_ROW];
    const RrJob job = jobs[blockIdx.x];
    const int64_t a = row_lo[job.epoch], b = a + RR_ROW;                       // the row is [a, b)
    for (int i = threadIdx.x; i < RR_ROW; i += RR_THREADS) s_row[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // everything that decides a branch around a shuffle or a ballot below is the same in all lanes of a wave
    for (int64_t r = (int64_t)job.begin + (threadIdx.x >> 6); r < job.end; r += RR_WAVES) {
        const mpn_rr_take take = takes[r];
        TensLayout L;
        if (!tens_layout(text, len, take.off, &L)) {
            if (lane == 0) rr_flag_bad(bad, r);
            continue;
        }
        if (text[take.off + 13] < MPN_RR_MIN_MQ) continue;
        const int64_t cs = take.chunk_start;
        // an I or S of n <= l_seq bases at p reaches [p - n, p + n)
        const bool good = tens_wave_ops_k<false>(text, L, take.pos, a - L.l_seq, b + L.l_seq, lane, [&](int32_t, uint32_t op, int64_t n, int64_t r0, int64_t q0) {
            // M and X: the bases inside the row, positions [s, e)
            {
                const bool mx = op == OP_M || op == OP_X;
                const int64_t s = r0 > a ? r0 : a, e = r0 + n < b ? r0 + n : b;
                const int64_t m = mx && e > s ? e - s : 0;
                unsigned long long wide = __ballot(m >= RR_WIDE);
                while (wide) {
                    const int j = __ffsll(wide) - 1;
                    wide &= wide - 1;
                    const int64_t S = __shfl(s, j), E = __shfl(e, j), R0 = __shfl(r0, j), Q0 = __shfl(q0, j);
                    for (int64_t p = S + lane; p < E; p += 64) {
                        const int c = rr_base_counts(text, L, Q0 + (p - R0), contig, contig_len, p);
                        if (c < 0) rr_flag_bad(bad, r);
                        else if (c) atomicAdd(&s_row[p - a], 1);
                    }
                }
                if (m > 0 && m < RR_WIDE)
                    for (int64_t p = s; p < e; ++p) {
                        const int c = rr_base_counts(text, L, q0 + (p - r0), contig, contig_len, p);
                        if (c < 0) rr_flag_bad(bad, r);
                        else if (c) atomicAdd(&s_row[p - a], 1);
                    }
            }
            // I, S and D: a range of positions, one operation after the other
            const bool ins = op == OP_I || op == OP_S, range = ins || op == OP_D;
            const int64_t ra = ins ? r0 - n : r0, rb = r0 + n;
            const int64_t s = ra > a ? ra : a, e = rb < b ? rb : b;
            bool cand = range && n > 0 && e > s && rr_in_region(r0, cs);
            if (cand) {
                const int before = rr_before_ok(contig, contig_len, r0);
                if (before < 0) rr_flag_bad(bad, r);
                cand = before == 1;
            }
            if (cand && ins && q0 + n > L.l_seq) { rr_flag_bad(bad, r); cand = false; }
            unsigned long long todo = __ballot(cand);
            while (todo) {
                const int j = __ffsll(todo) - 1;
                todo &= todo - 1;
                const int64_t S = __shfl(s, j), E = __shfl(e, j), N = __shfl(n, j), Q0 = __shfl(q0, j);
                const int INS = __shfl((int)ins, j);
                if (INS) {
                    bool low = false;                                           // this lane's share of the n qualities, kept across the steps
                    for (int64_t i = lane; i < N; i += 64) low = low || text[L.qual + Q0 + i] < MPN_RR_MIN_BQ;
                    if (__ballot(low)) continue;
                }
                for (int64_t p = S + lane; p < E; p += 64) atomicAdd(&s_row[p - a], 1);
            }
        });
        if (!good && lane == 0) rr_flag_bad(bad, r);
    }
    __syncthreads();
    int32_t *__restrict__ out = rows + (int64_t)job.epoch * RR_ROW;
    for (int i = threadIdx.x; i < RR_ROW; i += RR_THREADS) {
        const int32_t v = s_row[i];
        if (job.plain) { if (v) out[i] += v; }
        else if (v) atomicAdd(&out[i], v);
    }
}

struct RrAssignArgs {
    const int32_t *pos, *end, *win_begin, *win_start, *win_end;
    int64_t n;
    int32_t n_splits;
};

__global__ __launch_bounds__(256) void rr_assign_kernel(RrAssignArgs A, int32_t *__restrict__ assign, int32_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n * A.n_splits) return;
    const int32_t s = (int32_t)(i / A.n);
    const int64_t r = i - (int64_t)s * A.n;
    const int32_t w0 = A.win_begin[s], nw = A.win_begin[s + 1] - w0;
    const int32_t w = rr_assign_one(A.pos[r], A.end[r], nw, A.win_start + w0, A.win_end + w0);
    assign[i] = w < 0 ? -1 : w0 + w;
    if (w >= 0) atomicAdd(&count[w0 + w], 1);
}

// jobs[j]: a window that has reads, its split, and where its reads begin in the list
struct RrCompactJob { int32_t window, split; int64_t at; };

__global__ __launch_bounds__(256) void rr_compact_kernel(RrAssignArgs A, const int32_t *__restrict__ assign, const RrCompactJob *__restrict__ jobs,
                                                         int32_t *__restrict__ list) {
    __shared__ int s_sum[4];
    const int32_t w = jobs[blockIdx.x].window, s = jobs[blockIdx.x].split;
    int64_t at = jobs[blockIdx.x].at;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r0 = 0; r0 < A.n; r0 += 256) {
        const int64_t r = r0 + threadIdx.x;
        const bool mine = r < A.n && assign[(int64_t)s * A.n + r] == w;
        const unsigned long long votes = __ballot(mine);
        const int rank = __popcll(votes & ((1ull << lane) - 1));
        if (lane == 0) s_sum[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < 4; ++k) { if (k < wave) before += s_sum[k]; all += s_sum[k]; }
        if (mine) list[at + before + rank] = (int32_t)r;
        at += all;
        __syncthreads();
    }
}

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_rr_last_device_ms(double *records_ms, double *support_ms, double *assign_ms) {
    if (records_ms) *records_ms = tl_rr_ms[0];
    if (support_ms) *support_ms = tl_rr_ms[1];
    if (assign_ms) *assign_ms = tl_rr_ms[2];
}

extern "C" int32_t mpn_rr_records(const void *d_text, int64_t text_len, int64_t n, const mpn_bam_row *rows, mpn_rr_rec *recs) {
    tl_rr_ms[0] = 0;
    if (n < 0 || n > 0x7fffffff || text_len < 0 || (n > 0 && (!rows || !recs || !d_text))) {
        set_error("mpn_rr_records: bad arguments");
        return -2;
    }
    for (int64_t r = 0; r < n; ++r)
        if (rows[r].off < 0 || rows[r].off > text_len - mpn_bamw::BAMW_FIXED) {
            set_error("mpn_rr_records: row %lld does not lie inside the text", (long long)r);
            return -2;
        }
    if (n == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_bam_row> d_rows;
    DevBuf<mpn_rr_rec> d_recs;
    DevTimer tm;
    if (d_rows.upload(rows, (size_t)n, st) || d_recs.alloc((size_t)n) || tm.start(st)) return -1;
    hipLaunchKernelGGL(rr_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_text, text_len,
                       (const mpn_bam_row *)d_rows.p, n, d_recs.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st) || d_recs.download(recs, (size_t)n, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return tm.elapsed_ms(&tl_rr_ms[0]);
}

extern "C" int32_t mpn_rr_chunks(int64_t n, const int32_t *pos, int64_t *first, int64_t *chunk, int32_t *chunk_of) {
    if (n < 0 || !first || !chunk || *chunk < 0 || *first < -1 || (n > 0 && (!pos || !chunk_of))) {
        set_error("mpn_rr_chunks: bad arguments");
        return -2;
    }
    for (int64_t i = 0; i < n; ++i)
        if (pos[i] < 0) { set_error("mpn_rr_chunks: record %lld has a negative position", (long long)i); return -2; }
    rr_chunks_serial(n, pos, first, chunk, chunk_of);
    return 0;
}

extern "C" int32_t mpn_rr_support(const void *d_text, int64_t text_len, int64_t n, const mpn_rr_take *takes, const int64_t *reach, int64_t n_epochs,
                                  const int32_t *epoch_chunk, const int32_t *row_lo, const void *d_contig, int64_t contig_len, int32_t slice,
                                  void *d_rows, int64_t *bad_row, int64_t *n_split) {
    tl_rr_ms[1] = 0;
    if (n < 0 || n > 0x7ffffff0 || text_len < 0 || (n > 0 && (!takes || !reach || !d_text)) || n_epochs < 0 || n_epochs > (1 << 24) ||
        (n_epochs > 0 && (!epoch_chunk || !row_lo || !d_rows)) || contig_len <= 0 || contig_len > 0x7fffffff || !d_contig || slice < 0 || !bad_row) {
        set_error("mpn_rr_support: bad arguments");
        return -2;
    }
    for (int64_t r = 0; r < n; ++r)
        if (reach[r] < 0 || takes[r].off < 0 || takes[r].off > text_len - mpn_bamw::BAMW_FIXED ||
            (r > 0 && (takes[r].pos < takes[r - 1].pos || takes[r].chunk < takes[r - 1].chunk))) {
            set_error("mpn_rr_support: record %lld: the records are not in ascending position and chunk, do not lie inside the text, or a reach is negative",
                      (long long)r);
            return -2;
        }
    for (int64_t e = 1; e < n_epochs; ++e)
        if (epoch_chunk[e] <= epoch_chunk[e - 1]) { set_error("mpn_rr_support: the epochs are not in ascending order"); return -2; }
    *bad_row = -1;
    if (n_split) *n_split = 0;
    if (n == 0 || n_epochs == 0) return 0;
    if (slice == 0) slice = MPN_RR_SLICE;
    // The jobs.  A record adds inside [pos - l_seq, pos + span + l_seq): the records of the row [a, b) are those from the first whose
    // running maximum of pos + reach passes a to the last whose pos is below b + the largest reach, among those parsed by the epoch.
    std::vector<int64_t> far((size_t)n);
    int64_t max_reach = 0;
    {
        int64_t m = INT64_MIN;
        for (int64_t r = 0; r < n; ++r) {
            m = std::max(m, (int64_t)takes[r].pos + reach[r]);
            far[(size_t)r] = m;
            max_reach = std::max(max_reach, reach[r]);
        }
    }
    std::vector<RrJob> jobs;
    int64_t split = 0;
    for (int64_t e = 0; e < n_epochs; ++e) {
        const int64_t a = row_lo[e], b = a + RR_ROW;
        const int32_t k = epoch_chunk[e];
        const int64_t parsed = std::partition_point(takes, takes + n, [k](const mpn_rr_take &x) { return x.chunk <= k; }) - takes;
        const int64_t first = std::lower_bound(far.begin(), far.end(), a + 1) - far.begin();
        const int64_t reachable = std::partition_point(takes, takes + n, [b, max_reach](const mpn_rr_take &x) { return (int64_t)x.pos < b + max_reach; }) - takes;
        const int64_t last = std::min(parsed, reachable);
        if (first >= last) continue;
        const bool plain = last - first <= slice;
        split += plain ? 0 : 1;
        for (int64_t r = first; r < last; r += slice)
            jobs.push_back(RrJob{(int32_t)e, (int32_t)r, (int32_t)std::min<int64_t>(r + slice, last), plain ? 1 : 0});
    }
    if (n_split) *n_split = split;
    if (jobs.empty()) return 0;
    if (jobs.size() > 0x7fffffffu) { set_error("mpn_rr_support: too many jobs"); return -2; }
    hipStream_t st = 0;
    DevBuf<mpn_rr_take> d_takes;
    DevBuf<RrJob> d_jobs;
    DevBuf<int32_t> d_lo, d_bad;
    DevTimer tm;
    const int32_t none = 0x7fffffff;
    if (d_takes.upload(takes, (size_t)n, st) || d_jobs.upload(jobs.data(), jobs.size(), st) || d_lo.upload(row_lo, (size_t)n_epochs, st) ||
        d_bad.upload(&none, 1, st) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(rr_support_kernel, dim3((unsigned)jobs.size()), dim3(RR_THREADS), 0, st, (const uint8_t *)d_text, text_len,
                       (const mpn_rr_take *)d_takes.p, (const RrJob *)d_jobs.p, (const int32_t *)d_lo.p, (const uint8_t *)d_contig, contig_len,
                       (int32_t *)d_rows, d_bad.p);
    MPN_HIP_CHECK(hipGetLastError());
    int32_t bad = none;
    if (tm.stop(st) || d_bad.download(&bad, 1, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (bad != none) *bad_row = bad;
    return tm.elapsed_ms(&tl_rr_ms[1]);
}

extern "C" int32_t mpn_rr_assign(int64_t n, const int32_t *pos, const int32_t *end, int32_t n_splits, const int32_t *win_begin, const int32_t *win_start,
                                 const int32_t *win_end, int32_t *count, int32_t *list, int64_t cap) {
    tl_rr_ms[2] = 0;
    if (n < 0 || n > 0x7fffffff || n_splits < 0 || n_splits > 4096 || (n > 0 && (!pos || !end)) || (n_splits > 0 && !win_begin) || cap < 0 ||
        (cap > 0 && !list)) {
        set_error("mpn_rr_assign: bad arguments");
        return -2;
    }
    const int32_t n_win = n_splits > 0 ? win_begin[n_splits] : 0;
    if (n_splits > 0 && (win_begin[0] != 0 || n_win < 0 || n_win > (1 << 20) || (n_win > 0 && (!win_start || !win_end || !count)))) {
        set_error("mpn_rr_assign: bad arguments");
        return -2;
    }
    for (int32_t s = 0; s < n_splits; ++s) {
        if (win_begin[s + 1] < win_begin[s] || win_begin[s + 1] > n_win) { set_error("mpn_rr_assign: the window offsets do not ascend"); return -2; }
        for (int32_t w = win_begin[s]; w < win_begin[s + 1]; ++w)
            if (win_end[w] < win_start[w] || (w > win_begin[s] && win_start[w] < win_end[w - 1])) {
                set_error("mpn_rr_assign: the windows of split %d are not sorted and disjoint", s);
                return -2;
            }
    }
    for (int32_t w = 0; w < n_win; ++w) count[w] = 0;
    if (n == 0 || n_win == 0) return 0;
    if ((int64_t)n * n_splits > 0x7fffffff) { set_error("mpn_rr_assign: too many (split, read) pairs"); return -2; }
    hipStream_t st = 0;
    const int64_t pairs = n * n_splits;
    DevBuf<int32_t> d_pos, d_end, d_wb, d_ws, d_we, d_assign, d_count, d_list;
    DevTimer tm;
    if (d_pos.upload(pos, (size_t)n, st) || d_end.upload(end, (size_t)n, st) || d_wb.upload(win_begin, (size_t)n_splits + 1, st) ||
        d_ws.upload(win_start, (size_t)n_win, st) || d_we.upload(win_end, (size_t)n_win, st) || d_assign.alloc((size_t)pairs) ||
        d_count.alloc((size_t)n_win) || d_count.zero(st) || d_list.alloc((size_t)pairs) || tm.start(st))
        return -1;
    const RrAssignArgs A{d_pos.p, d_end.p, d_wb.p, d_ws.p, d_we.p, n, n_splits};
    hipLaunchKernelGGL(rr_assign_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, A, d_assign.p, d_count.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (d_count.download(count, (size_t)n_win, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    // the windows' offsets: one pass over the counts on the host
    std::vector<RrCompactJob> jobs;
    int64_t total = 0;
    for (int32_t s = 0; s < n_splits; ++s)
        for (int32_t w = win_begin[s]; w < win_begin[s + 1]; ++w) {
            if (count[w] < 0 || count[w] > n) { set_error("mpn_rr_assign: window %d counts %d reads", w, count[w]); return -1; }
            if (count[w] > 0) jobs.push_back(RrCompactJob{w, s, total});
            total += count[w];
        }
    if (total > pairs) { set_error("mpn_rr_assign: the counts add up to %lld", (long long)total); return -1; }
    DevBuf<RrCompactJob> d_jobs;
    if (d_jobs.upload(jobs.data(), jobs.size(), st)) return -1;
    if (!jobs.empty())
        hipLaunchKernelGGL(rr_compact_kernel, dim3((unsigned)jobs.size()), dim3(256), 0, st, A, (const int32_t *)d_assign.p,
                           (const RrCompactJob *)d_jobs.p, d_list.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (tm.elapsed_ms(&tl_rr_ms[2])) return -1;
    if (total > cap) { set_error("mpn_rr_assign: %lld reads do not fit %lld", (long long)total, (long long)cap); return -3; }
    if (d_list.download(list, (size_t)total, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}
