// The per-base pile-up of a sorted BAM whose text is resident, behind include/mpn_pileup.h.  Semantics: Clair's
// preprocess/ExtractVariantCandidates.py; the arithmetic shared with the host is csrc/pileup_core.h.
//
//   pile_records_kernel   a lane per record: pile_record over its CIGAR (fixed fields, S, T, the span, a status).
//   pile_counts_kernel    a workgroup per job.  A job is a tile of MPN_PILEUP_TILE positions of the window and a slice of the
//                         records that can reach it (a contiguous range of the sorted rows, planned on the host from pos and the
//                         running maximum of pos + span).  The tile's 7 x 2048 counters are in LDS.  A wave takes one record at
//                         a time: 64 operations per step, a lane each; two wave scans give every lane the reference and query
//                         offset of its operation, the wave stops at the first step that starts behind the tile.  An I or D is
//                         one LDS atomic of its lane.  The bases of an M, = or X clipped to the tile are taken by the whole
//                         wave, a base per lane, when they are 32 or more, and by the operation's own lane otherwise (ONT
//                         CIGARs are mostly runs of a few bases).  At the end the tile goes to HBM: a tile with one job adds
//                         without atomics (no other workgroup of the launch touches it), the jobs of a split tile add with
//                         atomicAdd.  Integer sums: the order does not show.
//   pile_flag_kernel / pile_offsets_kernel / pile_emit_kernel
//                         the candidate table.  A block of 256 threads decides 1024 positions (pile_decide, float64) and
//                         counts those that pass; one block scans the block counts; the blocks decide again and write their
//                         rows behind their offset, in position order.  No cursor, no atomics.
// The packed bases are read byte by byte (a base per lane): see profiles/r20_candidates/README.md for what that costs.
#include "mpn_common.h"
#include "pileup_core.h"

namespace mpn {

using namespace mpn_pile;

static thread_local double tl_pile_ms[3] = {0, 0, 0};     // device time of the last calls on this thread: records, counts, candidates

static_assert(sizeof(mpn_pileup_rec) == 40 && sizeof(mpn_pileup_take) == 16 && sizeof(mpn_pileup_cand) == 44, "the layouts the Python layer reads");
static_assert(MPN_PILEUP_TILE * MPN_PILEUP_SLOTS * 4 <= 64 * 1024 - 256, "the tile is static LDS");

constexpr int PILE_THREADS = 512, PILE_WAVES = PILE_THREADS / 64;
constexpr int PILE_WIDE = 32;          // clipped bases of one operation from which the whole wave takes them

struct PileJob { int32_t tile, begin, end, plain; };

// ---- records -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pile_records_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_bam_row *__restrict__ rows,
                                                           int64_t n, mpn_pileup_rec *__restrict__ recs) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    mpn_pileup_rec rec;
    pile_record(text, len, rows[r].off, &rec);       // (the host has checked off + 36 <= len)
    recs[r] = rec;
}

// ---- counts --------------------------------------------------------------------------------------------------------------------
// inclusive prefix sum over the wave in 64 bits (the lengths of 64 operations pass 32 bits)
__device__ __forceinline__ int64_t pile_scan64(int64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

__device__ __forceinline__ void pile_flag_bad(int32_t *bad, int64_t r) { atomicMin(bad, (int32_t)r); }

// one base of record r: query index q, tile slot index ti = (position - tile start)
__device__ __forceinline__ void pile_base(const uint8_t *__restrict__ text, const PileLayout &L, int64_t q, int64_t ti, int32_t *s_tile, int32_t *bad,
                                          int64_t r) {
    if (q >= L.l_seq) { pile_flag_bad(bad, r); return; }
    const uint32_t byte = text[L.seq + (q >> 1)];
    const int slot = pile_slot((q & 1) ? byte : byte >> 4);
    if (slot == PILE_NONE) { pile_flag_bad(bad, r); return; }
    atomicAdd(&s_tile[ti * MPN_PILEUP_SLOTS + slot], 1);
}

__global__ __launch_bounds__(PILE_THREADS) void pile_counts_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_pileup_take *__restrict__ takes,
                                                                   const PileJob *__restrict__ jobs, int64_t lo, int64_t hi,
                                                                   int32_t *__restrict__ counts, int32_t *__restrict__ bad) {
    __shared__ int32_t s_tile[MPN_PILEUP_TILE * MPN_PILEUP_SLOTS];
    const PileJob job = jobs[blockIdx.x];
    const int64_t a = lo + (int64_t)job.tile * MPN_PILEUP_TILE;                 // the tile is [a, b)
    const int64_t b = a + MPN_PILEUP_TILE < hi ? a + MPN_PILEUP_TILE : hi;
    for (int i = threadIdx.x; i < MPN_PILEUP_TILE * MPN_PILEUP_SLOTS; i += PILE_THREADS) s_tile[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // everything that decides a branch around a shuffle below is the same in all lanes of a wave
    for (int64_t r = (int64_t)job.begin + (threadIdx.x >> 6); r < job.end; r += PILE_WAVES) {
        const mpn_pileup_take take = takes[r];
        PileLayout L;
        if (!pile_layout(text, len, take.off, &L)) {
            if (lane == 0) pile_flag_bad(bad, r);
            continue;
        }
        const int64_t pos = take.pos;
        int64_t rbase = pos, qbase = 0;                                         // where the step's first operation starts
        for (int32_t k0 = 0; k0 < L.n_cigar && rbase <= b; k0 += 64) {          // (an operation that starts behind b adds at b or later)
            const int32_t k = k0 + lane;
            uint32_t op = OP_P, n = 0;
            if (k < L.n_cigar) {
                const uint32_t w = pile_u32(text, L.cigar + 4 * (int64_t)k);
                op = w & 15u; n = w >> 4;
            }
            if (op > 8) { pile_flag_bad(bad, r); op = OP_P; n = 0; }
            const bool match = pile_is_match(op);
            const int64_t radv = (match || op == OP_D) ? n : 0, qadv = (match || op == OP_I || op == OP_S) ? n : 0;
            const int64_t rincl = pile_scan64(radv, lane), qincl = pile_scan64(qadv, lane);
            const int64_t r0 = rbase + rincl - radv, q0 = qbase + qincl - qadv;
            rbase += __shfl(rincl, 63);
            qbase += __shfl(qincl, 63);
            if (op == OP_I || op == OP_D) {
                const int64_t p = r0 - 1;
                if ((r0 != pos || take.lead) && p >= a && p < b) atomicAdd(&s_tile[(p - a) * MPN_PILEUP_SLOTS + (op == OP_I ? PILE_I : PILE_D)], 1);
            }
            // the bases of the operation inside the tile: positions [s, e)
            const int64_t s = r0 > a ? r0 : a, e = r0 + (int64_t)n < b ? r0 + (int64_t)n : b;
            const int64_t m = match && e > s ? e - s : 0;
            unsigned long long wide = __ballot(m >= PILE_WIDE);
            while (wide) {
                const int j = __ffsll(wide) - 1;
                wide &= wide - 1;
                const int64_t S = __shfl(s, j), E = __shfl(e, j), R0 = __shfl(r0, j), Q0 = __shfl(q0, j);
                for (int64_t p = S + lane; p < E; p += 64) pile_base(text, L, Q0 + (p - R0), p - a, s_tile, bad, r);
            }
            if (m > 0 && m < PILE_WIDE)
                for (int64_t p = s; p < e; ++p) pile_base(text, L, q0 + (p - r0), p - a, s_tile, bad, r);
        }
    }
    __syncthreads();
    const int64_t cells = (b - a) * MPN_PILEUP_SLOTS;
    int32_t *__restrict__ out = counts + (a - lo) * MPN_PILEUP_SLOTS;
    for (int64_t i = threadIdx.x; i < cells; i += PILE_THREADS) {
        const int32_t v = s_tile[i];
        if (!v) continue;
        if (job.plain) out[i] += v; else atomicAdd(&out[i], v);
    }
}

// ---- candidates ----------------------------------------------------------------------------------------------------------------
constexpr int CAND_THREADS = 256, CAND_PER_THREAD = 4, CAND_BLOCK = CAND_THREADS * CAND_PER_THREAD;

struct CandArgs {
    const int32_t *counts; const uint8_t *ref; const int64_t *bed_start, *bed_end;
    int64_t lo, n_pos, n_bed;
    double min_coverage, threshold;
};

__device__ __forceinline__ bool cand_at(const CandArgs &A, int64_t i, mpn_pileup_cand *row) {
    if (i >= A.n_pos) return false;
    const int64_t p = A.lo + i;
    if (A.n_bed >= 0) {        // the last interval that starts at or before p
        int64_t x = 0, y = A.n_bed;
        while (x < y) {
            const int64_t mid = x + ((y - x) >> 1);
            if (A.bed_start[mid] <= p) x = mid + 1; else y = mid;
        }
        if (x == 0 || p >= A.bed_end[x - 1]) return false;
    }
    int32_t c[MPN_PILEUP_SLOTS];
#pragma unroll
    for (int k = 0; k < MPN_PILEUP_SLOTS; ++k) c[k] = A.counts[i * MPN_PILEUP_SLOTS + k];
    if (!pile_decide(c, A.ref[i], A.min_coverage, A.threshold, row)) return false;
    row->pos = (int32_t)p;
    return true;
}

__global__ __launch_bounds__(CAND_THREADS) void pile_flag_kernel(CandArgs A, int64_t *__restrict__ block_count) {
    __shared__ int s_sum[CAND_THREADS / 64];
    const int64_t i0 = ((int64_t)blockIdx.x * CAND_THREADS + threadIdx.x) * CAND_PER_THREAD;
    mpn_pileup_cand row;
    int c = 0;
    for (int k = 0; k < CAND_PER_THREAD; ++k) c += cand_at(A, i0 + k, &row) ? 1 : 0;
    const int w = wave_scan_add(c);
    if ((threadIdx.x & 63) == 63) s_sum[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < CAND_THREADS / 64; ++k) t += s_sum[k];
        block_count[blockIdx.x] = t;
    }
}

// one block: block_off[b] = the sum of block_count[0 .. b), block_off[n_blocks] = the total
__global__ __launch_bounds__(1024) void pile_offsets_kernel(const int64_t *__restrict__ block_count, int64_t n_blocks, int64_t *__restrict__ block_off) {
    __shared__ int64_t s_part[1024];
    const int64_t per = (n_blocks + 1023) / 1024, x0 = (int64_t)threadIdx.x * per, x1 = x0 + per < n_blocks ? x0 + per : n_blocks;
    int64_t sum = 0;
    for (int64_t x = x0; x < x1; ++x) sum += block_count[x];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t u = threadIdx.x >= d ? s_part[threadIdx.x - d] : 0;
        __syncthreads();
        s_part[threadIdx.x] += u;
        __syncthreads();
    }
    int64_t run = s_part[threadIdx.x] - sum;
    for (int64_t x = x0; x < x1; ++x) { block_off[x] = run; run += block_count[x]; }
    if (threadIdx.x == 1023) block_off[n_blocks] = s_part[1023];
}

__global__ __launch_bounds__(CAND_THREADS) void pile_emit_kernel(CandArgs A, const int64_t *__restrict__ block_off, mpn_pileup_cand *__restrict__ rows,
                                                                 int64_t cap) {
    __shared__ int s_sum[CAND_THREADS / 64];
    const int64_t i0 = ((int64_t)blockIdx.x * CAND_THREADS + threadIdx.x) * CAND_PER_THREAD;
    mpn_pileup_cand row[CAND_PER_THREAD];
    bool take[CAND_PER_THREAD];
    int c = 0;
#pragma unroll
    for (int k = 0; k < CAND_PER_THREAD; ++k) { take[k] = cand_at(A, i0 + k, &row[k]); c += take[k] ? 1 : 0; }
    const int w = wave_scan_add(c);
    if ((threadIdx.x & 63) == 63) s_sum[threadIdx.x >> 6] = w;
    __syncthreads();
    int64_t at = block_off[blockIdx.x] + (w - c);
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) at += s_sum[k];
#pragma unroll
    for (int k = 0; k < CAND_PER_THREAD; ++k)
        if (take[k]) {
            if (at < cap) rows[at] = row[k];
            ++at;
        }
}

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_pileup_last_device_ms(double *records_ms, double *counts_ms, double *candidates_ms) {
    if (records_ms) *records_ms = tl_pile_ms[0];
    if (counts_ms) *counts_ms = tl_pile_ms[1];
    if (candidates_ms) *candidates_ms = tl_pile_ms[2];
}

extern "C" int32_t mpn_pileup_records(const void *d_text, int64_t text_len, int64_t n, const mpn_bam_row *rows, mpn_pileup_rec *recs) {
    tl_pile_ms[0] = 0;
    if (n < 0 || n > 0x7fffffff || text_len < 0 || (n > 0 && (!rows || !recs || !d_text))) {
        set_error("mpn_pileup_records: bad arguments");
        return -2;
    }
    for (int64_t r = 0; r < n; ++r)
        if (rows[r].off < 0 || rows[r].off > text_len - mpn_bamw::BAMW_FIXED) {
            set_error("mpn_pileup_records: row %lld does not lie inside the text", (long long)r);
            return -2;
        }
    if (n == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_bam_row> d_rows;
    DevBuf<mpn_pileup_rec> d_recs;
    DevTimer tm;
    if (d_rows.upload(rows, (size_t)n, st) || d_recs.alloc((size_t)n) || tm.start(st)) return -1;
    hipLaunchKernelGGL(pile_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_text, text_len,
                       (const mpn_bam_row *)d_rows.p, n, d_recs.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st) || d_recs.download(recs, (size_t)n, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return tm.elapsed_ms(&tl_pile_ms[0]);
}

extern "C" int32_t mpn_pileup_counts(const void *d_text, int64_t text_len, int64_t n, const mpn_pileup_take *takes, const int64_t *span, int64_t lo,
                                     int64_t hi, int32_t slice, void *d_counts, int64_t *bad_row, int64_t *n_sliced) {
    tl_pile_ms[1] = 0;
    if (n < 0 || n > 0x7ffffff0 || text_len < 0 || (n > 0 && (!takes || !span || !d_text)) || lo < 0 || hi < lo || hi > 0x7fffffff || slice < 0 ||
        !bad_row || (hi > lo && !d_counts)) {
        set_error("mpn_pileup_counts: bad arguments");
        return -2;
    }
    for (int64_t r = 0; r < n; ++r)
        if (span[r] < 0 || (r > 0 && takes[r].pos < takes[r - 1].pos)) {
            set_error("mpn_pileup_counts: record %lld: the records are not in ascending position, or a span is negative", (long long)r);
            return -2;
        }
    *bad_row = -1;
    if (n_sliced) *n_sliced = 0;
    if (n == 0 || hi == lo) return 0;
    if (slice == 0) slice = MPN_PILEUP_SLICE;
    // The jobs.  A record adds at positions pos - 1 .. pos + span - 1: the records of the tile [a, b) are those from the first whose
    // running maximum of pos + span reaches a + 1 to the last whose pos is at most b.
    std::vector<int64_t> reach((size_t)n);
    {
        int64_t m = INT64_MIN;
        for (int64_t r = 0; r < n; ++r) { m = std::max(m, (int64_t)takes[r].pos + span[r]); reach[(size_t)r] = m; }
    }
    std::vector<PileJob> jobs;
    int64_t sliced = 0;
    const int64_t n_tiles = (hi - lo + MPN_PILEUP_TILE - 1) / MPN_PILEUP_TILE;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t a = lo + t * MPN_PILEUP_TILE, b = std::min(a + MPN_PILEUP_TILE, hi);
        const int64_t first = std::lower_bound(reach.begin(), reach.end(), a + 1) - reach.begin();
        const int64_t last = std::partition_point(takes, takes + n, [b](const mpn_pileup_take &x) { return (int64_t)x.pos <= b; }) - takes;
        if (first >= last) continue;
        const bool plain = last - first <= slice;
        sliced += plain ? 0 : 1;
        for (int64_t r = first; r < last; r += slice)
            jobs.push_back(PileJob{(int32_t)t, (int32_t)r, (int32_t)std::min<int64_t>(r + slice, last), plain ? 1 : 0});
    }
    if (n_sliced) *n_sliced = sliced;
    if (jobs.empty()) return 0;
    if (jobs.size() > 0x7fffffffu) { set_error("mpn_pileup_counts: too many jobs"); return -2; }
    hipStream_t st = 0;
    DevBuf<mpn_pileup_take> d_takes;
    DevBuf<PileJob> d_jobs;
    DevBuf<int32_t> d_bad;
    DevTimer tm;
    const int32_t none = 0x7fffffff;
    if (d_takes.upload(takes, (size_t)n, st) || d_jobs.upload(jobs.data(), jobs.size(), st) || d_bad.upload(&none, 1, st) || tm.start(st)) return -1;
    hipLaunchKernelGGL(pile_counts_kernel, dim3((unsigned)jobs.size()), dim3(PILE_THREADS), 0, st, (const uint8_t *)d_text, text_len,
                       (const mpn_pileup_take *)d_takes.p, (const PileJob *)d_jobs.p, lo, hi, (int32_t *)d_counts, d_bad.p);
    MPN_HIP_CHECK(hipGetLastError());
    int32_t bad = none;
    if (tm.stop(st) || d_bad.download(&bad, 1, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (bad != none) *bad_row = bad;
    return tm.elapsed_ms(&tl_pile_ms[1]);
}

extern "C" int32_t mpn_pileup_candidates(const void *d_counts, int64_t lo, int64_t n_pos, const uint8_t *ref, int64_t n_bed, const int64_t *bed_start,
                                         const int64_t *bed_end, double min_coverage, double threshold, int64_t cap, mpn_pileup_cand *rows,
                                         int64_t *n_rows) {
    tl_pile_ms[2] = 0;
    if (lo < 0 || n_pos < 0 || lo + n_pos > 0x7fffffff || (n_pos > 0 && (!d_counts || !ref)) || (n_bed > 0 && (!bed_start || !bed_end)) || cap < 0 ||
        (cap > 0 && !rows) || !n_rows || !(min_coverage > 0)) {
        set_error("mpn_pileup_candidates: bad arguments");
        return -2;
    }
    for (int64_t i = 0; i < n_bed; ++i)
        if (bed_end[i] <= bed_start[i] || (i > 0 && bed_start[i] < bed_end[i - 1])) {
            set_error("mpn_pileup_candidates: the intervals are not sorted and disjoint");
            return -2;
        }
    *n_rows = 0;
    if (n_pos == 0) return 0;
    hipStream_t st = 0;
    const int64_t n_blocks = (n_pos + CAND_BLOCK - 1) / CAND_BLOCK;
    DevBuf<uint8_t> d_ref;
    DevBuf<int64_t> d_bs, d_be, d_cnt, d_off;
    DevBuf<mpn_pileup_cand> d_rows;
    DevTimer tm;
    if (d_ref.upload(ref, (size_t)n_pos, st) || d_bs.upload(bed_start, (size_t)std::max<int64_t>(n_bed, 0), st) ||
        d_be.upload(bed_end, (size_t)std::max<int64_t>(n_bed, 0), st) || d_cnt.alloc((size_t)n_blocks) || d_off.alloc((size_t)n_blocks + 1) || tm.start(st))
        return -1;
    const CandArgs A{(const int32_t *)d_counts, d_ref.p, d_bs.p, d_be.p, lo, n_pos, n_bed < 0 ? -1 : n_bed, min_coverage, threshold};
    hipLaunchKernelGGL(pile_flag_kernel, dim3((unsigned)n_blocks), dim3(CAND_THREADS), 0, st, A, d_cnt.p);
    hipLaunchKernelGGL(pile_offsets_kernel, dim3(1), dim3(1024), 0, st, (const int64_t *)d_cnt.p, n_blocks, d_off.p);
    MPN_HIP_CHECK(hipGetLastError());
    int64_t total = 0;
    MPN_HIP_CHECK(hipMemcpyAsync(&total, d_off.p + n_blocks, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (total < 0 || total > n_pos) { set_error("mpn_pileup_candidates: the scan reported %lld rows", (long long)total); return -1; }
    *n_rows = total;
    if (total > cap) {
        if (tm.stop(st)) return -1;
        MPN_HIP_CHECK(hipStreamSynchronize(st));
        if (tm.elapsed_ms(&tl_pile_ms[2])) return -1;
        set_error("mpn_pileup_candidates: %lld rows do not fit %lld", (long long)total, (long long)cap);
        return -3;
    }
    if (total > 0) {
        if (d_rows.alloc((size_t)total)) return -1;
        hipLaunchKernelGGL(pile_emit_kernel, dim3((unsigned)n_blocks), dim3(CAND_THREADS), 0, st, A, (const int64_t *)d_off.p, d_rows.p, total);
        MPN_HIP_CHECK(hipGetLastError());
    }
    if (tm.stop(st) || d_rows.download(rows, (size_t)total, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return tm.elapsed_ms(&tl_pile_ms[2]);
}
