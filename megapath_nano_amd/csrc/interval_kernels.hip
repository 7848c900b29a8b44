// Sorting and interval-union kernels behind include/mpn_abundance.h: the coordinate sort of BAM records
// (`samtools sort`, /root/reference/bin/lib/aligner.py:246-252) and the covered base pairs per assembly
// (`bedtools sort | merge` + sum, /root/reference/bin/megapath_nano.py:313-347).  Byte/integer work bound by HBM traffic:
// a record is 24 bytes and a radix pass reads and writes it once (48 B per record and pass; constant digits are skipped).
#include "mpn_common.h"
#include "../../include/mpn_abundance.h"
#include "../../include/mpn_reads.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace mpn {

struct Rec3 { uint64_t hi, lo; int64_t idx; };

__device__ __forceinline__ uint32_t rec_digit(const Rec3 &r, int pass) {   // pass 0..7: bytes of lo, 8..15: bytes of hi
    return (uint32_t)((pass < 8 ? r.lo >> (8 * pass) : r.hi >> (8 * (pass - 8))) & 0xff);
}

constexpr int RS_THREADS = 256;

// per block: histogram of its chunk's digits -> hist[digit * n_blocks + block]; and which digits vary at all (any_diff)
__global__ __launch_bounds__(RS_THREADS) void rs_hist_kernel(const Rec3 *__restrict__ src, int64_t n, int64_t chunk, int pass,
                                                             uint32_t *__restrict__ hist, int n_blocks) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += RS_THREADS) atomicAdd(&h[rec_digit(src[i], pass)], 1u);
    __syncthreads();
    hist[(size_t)threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

// one block: exclusive scan of the digit-major table (256 * n_blocks entries); flag[0] = 1 if one digit holds every record
__global__ __launch_bounds__(1024) void rs_scan_kernel(uint32_t *__restrict__ hist, int n_blocks, int64_t n, int *__restrict__ flag) {
    __shared__ unsigned long long part[1024];
    __shared__ int single;
    const int total = 256 * n_blocks, t = threadIdx.x, per = (total + 1023) / 1024, lo = min(total, t * per), hi = min(total, lo + per);
    if (t == 0) single = 0;
    __syncthreads();
    unsigned long long s = 0;
    for (int k = lo; k < hi; ++k) s += hist[k];
    part[t] = s;
    // a digit that holds all n records: its row of the table sums to n
    if (t < 256) { unsigned long long d = 0; for (int b = 0; b < n_blocks; ++b) d += hist[(size_t)t * n_blocks + b]; if ((int64_t)d == n) single = 1; }
    __syncthreads();
    if (t == 0) { unsigned long long acc = 0; for (int k = 0; k < 1024; ++k) { const unsigned long long v = part[k]; part[k] = acc; acc += v; } flag[0] = single; }
    __syncthreads();
    if (single) return;
    unsigned long long o = part[t];
    for (int k = lo; k < hi; ++k) { const uint32_t v = hist[k]; hist[k] = (uint32_t)o; o += v; }
}

// stable scatter: the block walks its chunk in order, 256 records at a time; a record's slot = running offset of its digit
// + its rank among the earlier records of the tile with the same digit (ballots inside a wave, per-wave counts across waves)
__global__ __launch_bounds__(RS_THREADS) void rs_scatter_kernel(const Rec3 *__restrict__ src, Rec3 *__restrict__ dst, int64_t n, int64_t chunk,
                                                                int pass, const uint32_t *__restrict__ offs, int n_blocks, const int *__restrict__ flag) {
    if (flag[0]) return;   // constant digit: the pass is skipped (the host keeps src as the current buffer)
    __shared__ uint32_t bins[256], wcnt[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    bins[tid] = offs[(size_t)tid * n_blocks + blockIdx.x];
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (int64_t t0 = lo; t0 < hi; t0 += RS_THREADS) {
        const int64_t i = t0 + tid;
        const bool act = i < hi;
        Rec3 r{0, 0, 0};
        uint32_t dg = 0;
        if (act) { r = src[i]; dg = rec_digit(r, pass); }
        wcnt[0][tid] = 0; wcnt[1][tid] = 0; wcnt[2][tid] = 0; wcnt[3][tid] = 0;
        __syncthreads();
        unsigned long long same = __ballot(act);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot((dg >> b) & 1);
            same &= ((dg >> b) & 1) ? m : ~m;
        }
        const uint32_t rank = __popcll(same & ((1ULL << lane) - 1));
        if (act && rank == 0) wcnt[wv][dg] = __popcll(same);
        __syncthreads();
        if (act) {
            uint32_t o = bins[dg] + rank;
            for (int w2 = 0; w2 < wv; ++w2) o += wcnt[w2][dg];
            dst[o] = r;
        }
        __syncthreads();
        bins[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void rs_fill_kernel(const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo, int64_t n, Rec3 *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = Rec3{hi[i], lo[i], i};
}
__global__ __launch_bounds__(256) void rs_order_kernel(const Rec3 *__restrict__ rec, int64_t n, int64_t *__restrict__ order) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) order[i] = rec[i].idx;
}

// sorts d_a in place by (hi, lo), stable; d_b: bounce buffer of the same size.  Returns the buffer that holds the result.
// skip: bit p set = the caller knows that digit p is the same in every record, so pass p is not even counted.
static int radix_sort_rec3(Rec3 *d_a, Rec3 *d_b, int64_t n, Rec3 **result, hipStream_t st, uint32_t skip = 0) {
    *result = d_a;
    if (n < 2) return 0;
    const int n_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (n + 4095) / 4096));
    const int64_t chunk = (n + n_blocks - 1) / n_blocks;
    DevBuf<uint32_t> hist;
    DevBuf<int> flag;
    if (hist.alloc((size_t)256 * n_blocks) || flag.alloc(1)) return -1;
    int *h_flag = nullptr;
    MPN_HIP_CHECK(hipHostMalloc((void **)&h_flag, 64, hipHostMallocDefault));
    Rec3 *src = d_a, *dst = d_b;
    int rc = 0;
    for (int pass = 0; pass < 16 && !rc; ++pass) {
        if (skip >> pass & 1) continue;
        hipLaunchKernelGGL(rs_hist_kernel, dim3(n_blocks), dim3(RS_THREADS), 0, st, (const Rec3 *)src, n, chunk, pass, hist.p, n_blocks);
        hipLaunchKernelGGL(rs_scan_kernel, dim3(1), dim3(1024), 0, st, hist.p, n_blocks, n, flag.p);
        hipLaunchKernelGGL(rs_scatter_kernel, dim3(n_blocks), dim3(RS_THREADS), 0, st, (const Rec3 *)src, dst, n, chunk, pass, (const uint32_t *)hist.p, n_blocks,
                           (const int *)flag.p);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h_flag, flag.p, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { set_error("radix sort pass %d failed", pass); rc = -1; break; }
        if (!*h_flag) { Rec3 *t = src; src = dst; dst = t; }
    }
    (void)hipHostFree(h_flag);
    *result = src;
    return rc;
}

// ---- union length of intervals per (group, sequence), summed per group ----------------------------------------------------
// records sorted by (hi = group << 32 | seq, lo = start << 32 | end).  A thread sweeps one chunk of the sorted list; the running
// interval that enters a chunk comes from a serial pass over the chunk summaries (phase 2), like a three-phase scan.
struct SweepSum { uint64_t first_key, last_key; uint32_t run_end; int32_t one_key; };

__global__ __launch_bounds__(256) void cov_phase1_kernel(const Rec3 *__restrict__ rec, int64_t n, int64_t chunk, int n_chunks, SweepSum *__restrict__ sums) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const int64_t lo = (int64_t)c * chunk, hi = lo + chunk < n ? lo + chunk : n;
    SweepSum s{0, 0, 0, 1};
    if (lo < hi) {
        s.first_key = rec[lo].hi;
        uint64_t key = s.first_key;
        uint32_t run_end = 0;
        for (int64_t i = lo; i < hi; ++i) {
            const Rec3 r = rec[i];
            if (r.hi != key) { key = r.hi; run_end = 0; s.one_key = 0; }
            const uint32_t e = (uint32_t)r.lo;
            run_end = e > run_end ? e : run_end;
        }
        s.last_key = key; s.run_end = run_end;
    }
    sums[c] = s;
}

// carry[c] = (key, running end) of the interval group that is open when chunk c starts (key = ~0: none)
__global__ void cov_phase2_kernel(const SweepSum *__restrict__ sums, int n_chunks, uint64_t *__restrict__ carry_key, uint32_t *__restrict__ carry_end) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t key = ~0ULL;
    uint32_t end = 0;
    for (int c = 0; c < n_chunks; ++c) {
        carry_key[c] = key; carry_end[c] = end;
        const SweepSum s = sums[c];
        if (s.one_key && s.first_key == key) end = s.run_end > end ? s.run_end : end;   // the open group runs through the whole chunk
        else { key = s.last_key; end = s.run_end; }
        // (one_key with another key, or several keys: the chunk's last group is the open one, with the chunk's own running end --
        //  unless that last group started before the chunk, which only happens in the one_key case handled above)
    }
}

__global__ __launch_bounds__(256) void cov_phase3_kernel(const Rec3 *__restrict__ rec, int64_t n, int64_t chunk, int n_chunks,
                                                         const uint64_t *__restrict__ carry_key, const uint32_t *__restrict__ carry_end,
                                                         unsigned long long *__restrict__ covered, int32_t n_groups) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const int64_t lo = (int64_t)c * chunk, hi = lo + chunk < n ? lo + chunk : n;
    uint64_t key = carry_key[c];
    uint32_t run_end = carry_end[c];
    unsigned long long acc = 0;
    uint32_t acc_group = 0xffffffffu;
    for (int64_t i = lo; i < hi; ++i) {
        const Rec3 r = rec[i];
        const uint32_t s = (uint32_t)(r.lo >> 32), e = (uint32_t)r.lo, g = (uint32_t)(r.hi >> 32);
        if (g != acc_group) {
            if (acc && acc_group < (uint32_t)n_groups) atomicAdd(&covered[acc_group], acc);
            acc = 0; acc_group = g;
        }
        if (r.hi != key) { key = r.hi; run_end = 0; acc += e - s; run_end = e; continue; }
        // same (group, sequence): overlapping and book-ended intervals merge (start <= running end)
        if (s > run_end) acc += e - s;
        else if (e > run_end) acc += e - run_end;
        run_end = e > run_end ? e : run_end;
    }
    if (acc && acc_group < (uint32_t)n_groups) atomicAdd(&covered[acc_group], acc);
}


// ---- depth profile, depth BED and depth span per key (`bedtools genomecov -bg`, threshold, `sort | merge`) ------------------
// Every contributing interval becomes two events {hi = key, lo = position, idx = +1 / -1}; an interval that contributes nothing
// becomes two events of weight 0.  After the sort by (key, position) the sweep is two three-phase scans with a lane per element:
//   A  events -> points: D = inclusive sum of the weights.  Every key's weights sum to zero, so the plain, unsegmented sum is the
//      depth on the key.  The last event of a (key, position) run carries the depth after that position; these events are
//      compacted, in order, into points (key, position, depth).
//   B  points -> rows and BED: with a = depth after point j and b = depth before it (the depth of point j - 1; 0 at j = 0 and,
//      by the zero sums, at the first point of every key), a row starts at j iff a > 0 and a != b and one ends there iff b > 0
//      and a != b; a BED interval starts iff a passes the group's range and b does not, and ends iff b passes and a does not.
//      Starts and ends pair up in order, so the k-th start and the k-th end fill the k-th output row from different lanes and no
//      lane has to look for the other side of its row.  span[g] = sum of the BED ends - sum of the BED starts.
// Each phase: per-tile totals (count), one block that turns them into tile bases (prefix), a rescan that writes (fill).
constexpr int DP_THREADS = 256, DP_ITEMS = MPN_DEPTH_TILE / DP_THREADS;
static_assert(MPN_DEPTH_TILE % DP_THREADS == 0 && MPN_DEPTH_TILE < 65536, "a tile is whole blocks of lanes, and two tile counts share an int");

// inclusive prefix sums of a and b over the block's 256 lanes: the DPP ladder in a wave, the 4 wave totals through ws[2][4].
// ta, tb: the block's sums.  One barrier; the caller alternates between two ws so that the next call needs no second one.
__device__ __forceinline__ void block_scan_add2(int &a, int &b, int (*ws)[4], int &ta, int &tb) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    a = wave_scan_add(a);
    b = wave_scan_add(b);
    if (lane == 63) { ws[0][wv] = a; ws[1][wv] = b; }
    __syncthreads();
    int pa = 0, pb = 0;
    ta = 0; tb = 0;
#pragma unroll
    for (int w = 0; w < DP_THREADS / 64; ++w) {
        const int sa = ws[0][w], sb = ws[1][w];
        if (w < wv) { pa += sa; pb += sb; }
        ta += sa; tb += sb;
    }
    a += pa; b += pb;
}

__global__ __launch_bounds__(256) void dp_events_kernel(const int32_t *__restrict__ key, const int64_t *__restrict__ start, const int64_t *__restrict__ end,
                                                        int64_t n, const int64_t *__restrict__ key_len, Rec3 *__restrict__ ev) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t k = key[i];
        const int64_t len = key_len[k], s = start[i], e = end[i] < len ? end[i] : len;   // the clip; s >= len then gives s >= e
        const bool on = s < e;
        ev[2 * i] = Rec3{(uint64_t)(uint32_t)k, on ? (uint64_t)s : 0, on ? 1 : 0};
        ev[2 * i + 1] = Rec3{(uint64_t)(uint32_t)k, on ? (uint64_t)e : 0, on ? -1 : 0};
    }
}

// the last event of its (key, position) run
__device__ __forceinline__ bool dp_run_ends(const Rec3 *__restrict__ ev, int64_t i, int64_t m, const Rec3 &r) {
    if (i + 1 == m) return true;
    return ev[i + 1].hi != r.hi || ev[i + 1].lo != r.lo;
}

// part[0 * nb + tile] = sum of the tile's weights, part[1 * nb + tile] = number of points the tile yields
__global__ __launch_bounds__(DP_THREADS) void dp_point_count_kernel(const Rec3 *__restrict__ ev, int64_t m, int32_t *__restrict__ part, int nb) {
    __shared__ int ws[2][4];
    const int64_t base = (int64_t)blockIdx.x * MPN_DEPTH_TILE;
    int d = 0, t = 0;
#pragma unroll
    for (int k = 0; k < DP_ITEMS; ++k) {
        const int64_t i = base + k * DP_THREADS + threadIdx.x;
        if (i < m) { const Rec3 r = ev[i]; d += (int)r.idx; t += dp_run_ends(ev, i, m, r); }
    }
    int td, tt;
    block_scan_add2(d, t, ws, td, tt);
    if (threadIdx.x == 0) { part[blockIdx.x] = td; part[(size_t)nb + blockIdx.x] = tt; }
}

// one block: exclusive scan, in place, of each of the nq rows of part[nq][nb]; total[q] = the sum of row q
__global__ __launch_bounds__(1024) void dp_prefix_kernel(int32_t *__restrict__ part, int nb, int nq, int32_t *__restrict__ total) {
    __shared__ int ws[2][16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, per = (nb + 1023) / 1024, lo = min(nb, t * per), hi = min(nb, lo + per);
    for (int q = 0; q < nq; ++q) {
        int32_t *row = part + (size_t)q * nb;
        int s = 0;
        for (int k = lo; k < hi; ++k) s += row[k];
        const int inc = wave_scan_add(s);
        if (lane == 63) ws[q & 1][wv] = inc;
        __syncthreads();
        int o = inc - s, all = 0;
        for (int w = 0; w < 16; ++w) { const int v = ws[q & 1][w]; if (w < wv) o += v; all += v; }
        for (int k = lo; k < hi; ++k) { const int v = row[k]; row[k] = o; o += v; }
        if (t == 0) total[q] = all;
    }
}

__global__ __launch_bounds__(DP_THREADS) void dp_point_fill_kernel(const Rec3 *__restrict__ ev, int64_t m, const int32_t *__restrict__ part, int nb,
                                                                   int32_t *__restrict__ pkey, uint32_t *__restrict__ ppos, int32_t *__restrict__ pdepth) {
    __shared__ int ws[2][2][4];
    const int64_t base = (int64_t)blockIdx.x * MPN_DEPTH_TILE;
    int run_d = part[blockIdx.x], run_t = part[(size_t)nb + blockIdx.x];
#pragma unroll
    for (int k = 0; k < DP_ITEMS; ++k) {
        if (base + k * DP_THREADS >= m) break;   // (the whole block leaves together)
        const int64_t i = base + k * DP_THREADS + threadIdx.x;
        Rec3 r{0, 0, 0};
        int ends = 0;
        if (i < m) { r = ev[i]; ends = dp_run_ends(ev, i, m, r); }
        int d = (int)r.idx, t = ends, td, tt;
        block_scan_add2(d, t, ws[k & 1], td, tt);
        if (ends) {
            const int64_t o = (int64_t)(uint32_t)(run_t + t - 1);
            pkey[o] = (int32_t)r.hi; ppos[o] = (uint32_t)r.lo; pdepth[o] = run_d + d;
        }
        run_d += td; run_t += tt;
    }
}

struct DpPoint { int32_t a, g; bool row_start, row_end, bed_start, bed_end; };

__device__ __forceinline__ DpPoint dp_classify(int64_t j, const int32_t *__restrict__ pkey, const int32_t *__restrict__ pdepth, const int32_t *__restrict__ key_group,
                                               const int32_t *__restrict__ dlo, const int32_t *__restrict__ dhi) {
    DpPoint p;
    p.a = pdepth[j];
    const int32_t b = j ? pdepth[j - 1] : 0;
    p.g = key_group[pkey[j]];
    const int32_t lo = dlo ? dlo[p.g] : 1, hi = dhi ? dhi[p.g] : 0x7fffffff;
    const bool pa = p.a > 0 && lo <= p.a && p.a <= hi, pb = b > 0 && lo <= b && b <= hi;
    p.row_start = p.a > 0 && p.a != b; p.row_end = b > 0 && p.a != b;
    p.bed_start = pa && !pb; p.bed_end = pb && !pa;
    return p;
}

// part[q * nb + tile], q = 0..3: row starts, row ends, BED starts, BED ends among the tile's points.  n_points: on the device
__global__ __launch_bounds__(DP_THREADS) void dp_row_count_kernel(const int32_t *__restrict__ pkey, const int32_t *__restrict__ pdepth, const int32_t *__restrict__ n_points,
                                                                  const int32_t *__restrict__ key_group, const int32_t *__restrict__ dlo, const int32_t *__restrict__ dhi,
                                                                  int32_t *__restrict__ part, int nb) {
    __shared__ int ws[2][4];
    const int64_t np = (uint32_t)n_points[0], base = (int64_t)blockIdx.x * MPN_DEPTH_TILE;
    int rows = 0, beds = 0;   // starts in the low half, ends in the high half: a tile has fewer than 2^16 of either
#pragma unroll
    for (int k = 0; k < DP_ITEMS; ++k) {
        const int64_t j = base + k * DP_THREADS + threadIdx.x;
        if (j < np) {
            const DpPoint p = dp_classify(j, pkey, pdepth, key_group, dlo, dhi);
            rows += (int)p.row_start | (int)p.row_end << 16;
            beds += (int)p.bed_start | (int)p.bed_end << 16;
        }
    }
    int tr, tb;
    block_scan_add2(rows, beds, ws, tr, tb);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = tr & 0xffff; part[(size_t)nb + blockIdx.x] = (uint32_t)tr >> 16;
        part[(size_t)2 * nb + blockIdx.x] = tb & 0xffff; part[(size_t)3 * nb + blockIdx.x] = (uint32_t)tb >> 16;
    }
}

// the row_* / bed_* lists and span may be null (not wanted)
__global__ __launch_bounds__(DP_THREADS) void dp_row_fill_kernel(const int32_t *__restrict__ pkey, const uint32_t *__restrict__ ppos, const int32_t *__restrict__ pdepth,
                                                                 const int32_t *__restrict__ n_points, const int32_t *__restrict__ key_group,
                                                                 const int32_t *__restrict__ dlo, const int32_t *__restrict__ dhi, const int32_t *__restrict__ part, int nb,
                                                                 int32_t *__restrict__ row_key, int64_t *__restrict__ row_start, int64_t *__restrict__ row_end,
                                                                 int32_t *__restrict__ row_depth, int32_t *__restrict__ bed_key, int64_t *__restrict__ bed_start,
                                                                 int64_t *__restrict__ bed_end, unsigned long long *__restrict__ span) {
    __shared__ int ws[2][2][4];
    const int64_t np = (uint32_t)n_points[0], base = (int64_t)blockIdx.x * MPN_DEPTH_TILE;
    const int64_t o_rs = (uint32_t)part[blockIdx.x], o_re = (uint32_t)part[(size_t)nb + blockIdx.x];
    const int64_t o_bs = (uint32_t)part[(size_t)2 * nb + blockIdx.x], o_be = (uint32_t)part[(size_t)3 * nb + blockIdx.x];
    int run_r = 0, run_b = 0;
#pragma unroll
    for (int k = 0; k < DP_ITEMS; ++k) {
        if (base + k * DP_THREADS >= np) break;   // (the whole block leaves together)
        const int64_t j = base + k * DP_THREADS + threadIdx.x;
        DpPoint p{0, 0, false, false, false, false};
        if (j < np) p = dp_classify(j, pkey, pdepth, key_group, dlo, dhi);
        int rows = (int)p.row_start | (int)p.row_end << 16, beds = (int)p.bed_start | (int)p.bed_end << 16, tr, tb;
        block_scan_add2(rows, beds, ws[k & 1], tr, tb);
        rows += run_r; beds += run_b;
        if (p.row_start | p.row_end | p.bed_start | p.bed_end) {
            const int64_t pos = ppos[j];
            if (row_key) {
                if (p.row_start) { const int64_t o = o_rs + (rows & 0xffff) - 1; row_key[o] = pkey[j]; row_start[o] = pos; row_depth[o] = p.a; }
                if (p.row_end) row_end[o_re + ((uint32_t)rows >> 16) - 1] = pos;
            }
            if (bed_key) {
                if (p.bed_start) { const int64_t o = o_bs + (beds & 0xffff) - 1; bed_key[o] = pkey[j]; bed_start[o] = pos; }
                if (p.bed_end) bed_end[o_be + ((uint32_t)beds >> 16) - 1] = pos;
            }
            // integer adds commute and wrap, so ends minus starts is exact in any order
            if (span && (p.bed_start | p.bed_end)) atomicAdd(&span[p.g], (unsigned long long)(p.bed_end ? pos : -pos));
        }
        run_r += tr; run_b += tb;
    }
}

// ---- union of a BED with the merged intervals as output, and the covered length of query intervals ---------------------------
// (`bedtools sort | merge`, and the counting half of `bedtools annotate`).  Records {hi = key + 1, lo = start << 32 | end} of the
// non-empty intervals, sorted by (key, start).  With v = (key + 1) << 32 | end, the plain running maximum of v is the running
// maximum of `end` on the current key, because the key field dominates and never decreases; P = that maximum over the records
// before record i (0: none), Q = max(P, v_i).  Record i heads a merged interval iff P is of another key or start_i > end(P)
// (touching merges); it is the tail of one iff record i + 1 is a head or there is none, and then end(Q) is the interval's end.
// Heads and tails alternate, so the k-th head and the k-th tail fill the k-th output row from their own lanes.  The same scan
// carries c = (tail ? end : 0) - (head ? start : 0): its sum over the records before a head is the summed length of the merged
// intervals before this one -- the exclusive prefix that the search below needs -- and its sum per group is span[g].
// Phases, a lane per record over tiles of MPN_BED_TILE: tile maxima; one block turns them into the maximum that enters each
// tile; heads and c per tile; one block turns those into tile bases; the rescan that writes.
constexpr int BU_THREADS = 256, BU_ITEMS = MPN_BED_TILE / BU_THREADS;
static_assert(MPN_BED_TILE % BU_THREADS == 0, "a tile is whole blocks of lanes");

__device__ __forceinline__ uint64_t wave_scan_max64(uint64_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)v, d);
        if (lane >= d && o > v) v = o;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_scan_add64(uint64_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ uint64_t bu_value(const Rec3 &r) { return r.hi << 32 | (uint32_t)r.lo; }

__global__ __launch_bounds__(BU_THREADS) void bu_tile_max_kernel(const Rec3 *__restrict__ rec, int64_t n, uint64_t *__restrict__ tmax) {
    __shared__ uint64_t ws[4];
    const int64_t base = (int64_t)blockIdx.x * MPN_BED_TILE;
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < BU_ITEMS; ++k) {
        const int64_t i = base + k * BU_THREADS + threadIdx.x;
        if (i < n) { const uint64_t x = bu_value(rec[i]); v = x > v ? x : v; }
    }
    v = wave_scan_max64(v);
    if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t m = 0;
        for (int w = 0; w < BU_THREADS / 64; ++w) m = ws[w] > m ? ws[w] : m;
        tmax[blockIdx.x] = m;
    }
}

// one block, in place: exclusive scans over the nb tiles.  is_max: the running maximum (identity 0); otherwise nq rows of sums,
// total[q] = the sum of row q
__global__ __launch_bounds__(1024) void bu_prefix_kernel(uint64_t *__restrict__ part, int nb, int nq, int is_max, uint64_t *__restrict__ total) {
    __shared__ uint64_t sh[1024];
    const int t = threadIdx.x, per = (nb + 1023) / 1024, lo = min(nb, t * per), hi = min(nb, lo + per);
    for (int q = 0; q < nq; ++q) {
        uint64_t *row = part + (size_t)q * nb;
        uint64_t s = 0;
        for (int k = lo; k < hi; ++k) s = is_max ? (row[k] > s ? row[k] : s) : s + row[k];
        sh[t] = s;
        __syncthreads();
        if (t == 0) {
            uint64_t acc = 0;
            for (int k = 0; k < 1024; ++k) { const uint64_t v = sh[k]; sh[k] = acc; acc = is_max ? (v > acc ? v : acc) : acc + v; }
            if (total) total[q] = acc;
        }
        __syncthreads();
        uint64_t o = sh[t];
        for (int k = lo; k < hi; ++k) { const uint64_t v = row[k]; row[k] = o; o = is_max ? (v > o ? v : o) : o + v; }
        __syncthreads();
    }
}

struct BuItem { bool head, tail; uint32_t key, start, end; };   // end: the end of the merged interval (meaningful at a tail)

// One step of the running maximum over the block's 256 records i = first + lane; run: the maximum over everything before
// `first`, moved on to include these records.  Every lane of the block calls it (one barrier); ws alternates between steps.
__device__ __forceinline__ BuItem bu_step(const Rec3 *__restrict__ rec, int64_t i, int64_t n, uint64_t &run, uint64_t *ws) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool act = i < n;
    Rec3 r{0, 0, 0};
    if (act) r = rec[i];
    const uint64_t v = act ? bu_value(r) : 0;
    const uint64_t inc = wave_scan_max64(v);
    if (lane == 63) ws[wv] = inc;
    uint64_t p = (uint64_t)__shfl_up((unsigned long long)inc, 1);
    if (lane == 0) p = 0;
    __syncthreads();
    uint64_t before = run, all = run;
#pragma unroll
    for (int w = 0; w < BU_THREADS / 64; ++w) {
        const uint64_t t = ws[w];
        if (w < wv && t > before) before = t;
        if (t > all) all = t;
    }
    run = all;
    p = before > p ? before : p;
    const uint64_t q = v > p ? v : p;
    BuItem it{false, false, (uint32_t)r.hi - 1, (uint32_t)(r.lo >> 32), (uint32_t)q};
    if (act) {
        it.head = (p >> 32) != r.hi || it.start > (uint32_t)p;
        it.tail = true;
        if (i + 1 < n) { const Rec3 nx = rec[i + 1]; it.tail = nx.hi != r.hi || (uint32_t)(nx.lo >> 32) > it.end; }
    }
    return it;
}

__device__ __forceinline__ uint64_t bu_contribution(const BuItem &it) { return (it.tail ? (uint64_t)it.end : 0) - (it.head ? (uint64_t)it.start : 0); }

// part[0 * nb + tile] = heads in the tile, part[1 * nb + tile] = sum of c over the tile (wrapping; the prefixes are exact)
__global__ __launch_bounds__(BU_THREADS) void bu_count_kernel(const Rec3 *__restrict__ rec, int64_t n, const uint64_t *__restrict__ tmax,
                                                              uint64_t *__restrict__ part, int nb) {
    __shared__ uint64_t wsm[2][4], wsa[2][4];
    const int64_t base = (int64_t)blockIdx.x * MPN_BED_TILE;
    uint64_t run = tmax[blockIdx.x], heads = 0, c = 0;
#pragma unroll
    for (int k = 0; k < BU_ITEMS; ++k) {
        if (base + k * BU_THREADS >= n) break;   // (the whole block leaves together)
        const BuItem it = bu_step(rec, base + k * BU_THREADS + threadIdx.x, n, run, wsm[k & 1]);
        heads += it.head; c += bu_contribution(it);
    }
    heads = wave_scan_add64(heads); c = wave_scan_add64(c);
    if ((threadIdx.x & 63) == 63) { wsa[0][threadIdx.x >> 6] = heads; wsa[1][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[blockIdx.x] = wsa[0][0] + wsa[0][1] + wsa[0][2] + wsa[0][3];
        part[(size_t)nb + blockIdx.x] = wsa[1][0] + wsa[1][1] + wsa[1][2] + wsa[1][3];
    }
}

// m_key / m_start / m_end / m_before: the merged intervals and the summed length of those before each; span may be null
__global__ __launch_bounds__(BU_THREADS) void bu_fill_kernel(const Rec3 *__restrict__ rec, int64_t n, const uint64_t *__restrict__ tmax,
                                                             const uint64_t *__restrict__ part, int nb, const int32_t *__restrict__ key_group,
                                                             int32_t *__restrict__ m_key, uint32_t *__restrict__ m_start, uint32_t *__restrict__ m_end,
                                                             uint64_t *__restrict__ m_before, unsigned long long *__restrict__ span) {
    __shared__ uint64_t wsm[2][4], wsa[2][2][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * MPN_BED_TILE;
    uint64_t run = tmax[blockIdx.x], run_heads = part[blockIdx.x], run_c = part[(size_t)nb + blockIdx.x];
#pragma unroll
    for (int k = 0; k < BU_ITEMS; ++k) {
        if (base + k * BU_THREADS >= n) break;   // (the whole block leaves together)
        const BuItem it = bu_step(rec, base + k * BU_THREADS + threadIdx.x, n, run, wsm[k & 1]);
        const uint64_t c = bu_contribution(it);
        uint64_t heads = wave_scan_add64(it.head), sum = wave_scan_add64(c);
        if (lane == 63) { wsa[k & 1][0][wv] = heads; wsa[k & 1][1][wv] = sum; }
        __syncthreads();
        uint64_t th = 0, tc = 0;
#pragma unroll
        for (int w = 0; w < BU_THREADS / 64; ++w) {
            const uint64_t a = wsa[k & 1][0][w], b = wsa[k & 1][1][w];
            if (w < wv) { heads += a; sum += b; }
            th += a; tc += b;
        }
        heads += run_heads; sum += run_c;          // inclusive, over the whole list
        if (it.head) { const uint64_t o = heads - 1; m_key[o] = (int32_t)it.key; m_start[o] = it.start; m_before[o] = sum - c; }
        if (it.tail) m_end[heads - 1] = it.end;
        // integer adds commute and wrap, so ends minus starts is exact in any order
        if (span && c) atomicAdd(&span[key_group[it.key]], (unsigned long long)c);
        run_heads += th; run_c += tc;
    }
}

// key_off[k], k in [0, n_keys]: the first merged interval whose key is >= k (the merged list is ordered by key)
__global__ __launch_bounds__(256) void bu_key_offsets_kernel(const int32_t *__restrict__ m_key, const uint64_t *__restrict__ n_merged, int32_t n_keys,
                                                             uint32_t *__restrict__ key_off) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_keys) return;
    uint32_t lo = 0, hi = (uint32_t)n_merged[0];
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (m_key[mid] < k) lo = mid + 1; else hi = mid; }
    key_off[k] = lo;
}

// A lane per query, two binary searches inside the key's segment of the merged list: a = the first interval that ends after
// q_start, b = the last that starts before q_end.  The intervals of a key are disjoint and do not touch, so ends and starts are
// both ascending and a..b are exactly the intervals that meet the query; only a and b can stick out of it.
// Each step is a dependent read that misses the caches for a large BED: the kernel holds a handful of registers and no LDS, so
// a SIMD keeps its 8 waves and the latency is hidden by the other waves' searches.
__global__ __launch_bounds__(256) void bu_cover_kernel(const int32_t *__restrict__ q_key, const int64_t *__restrict__ q_start, const int64_t *__restrict__ q_end, int64_t n_q,
                                                       const uint32_t *__restrict__ key_off, const uint32_t *__restrict__ m_start, const uint32_t *__restrict__ m_end,
                                                       const uint64_t *__restrict__ m_before, int64_t *__restrict__ covered) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t k = q_key[i];
        const uint32_t qs = (uint32_t)q_start[i], qe = (uint32_t)q_end[i];
        const uint32_t seg_lo = key_off[k], seg_hi = key_off[k + 1];
        uint32_t lo = seg_lo, hi = seg_hi;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (m_end[mid] <= qs) lo = mid + 1; else hi = mid; }
        const uint32_t a = lo;
        hi = seg_hi;                                   // the first interval at or after a that starts at or after q_end
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (m_start[mid] < qe) lo = mid + 1; else hi = mid; }
        int64_t c = 0;
        if (lo > a) {
            const uint32_t b = lo - 1, sa = m_start[a], sb = m_start[b], eb = m_end[b];
            c = (int64_t)(m_before[b] + (eb - sb) - m_before[a]) - (qs > sa ? qs - sa : 0) - (eb > qe ? eb - qe : 0);
        }
        covered[i] = c;
    }
}

// The merged list of a BED on the device.
struct BedUnion {
    DevBuf<Rec3> a, b;
    DevBuf<uint64_t> tmax, part, total;   // total[0] = the number of merged intervals, total[1] = their summed length
    DevBuf<int32_t> m_key;
    DevBuf<uint32_t> m_start, m_end;
    DevBuf<uint64_t> m_before;
};

// hi / lo: the packed records of the n >= 1 non-empty intervals; skip: as in radix_sort_rec3.  Everything is queued on st.
static int bed_union_on_device(BedUnion &u, const std::vector<uint64_t> &hi, const std::vector<uint64_t> &lo, uint32_t skip, const int32_t *d_key_group,
                               unsigned long long *d_span, hipStream_t st) {
    const int64_t n = (int64_t)hi.size();
    DevBuf<uint64_t> d_hi, d_lo;
    if (d_hi.upload(hi.data(), (size_t)n, st) || d_lo.upload(lo.data(), (size_t)n, st) || u.a.alloc((size_t)n) || u.b.alloc((size_t)n)) return -1;
    const int g = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 16));
    hipLaunchKernelGGL(rs_fill_kernel, dim3(g), dim3(256), 0, st, (const uint64_t *)d_hi.p, (const uint64_t *)d_lo.p, n, u.a.p);
    MPN_HIP_CHECK(hipGetLastError());
    Rec3 *rec = nullptr;
    if (radix_sort_rec3(u.a.p, u.b.p, n, &rec, st, skip)) return -1;
    const int nb = (int)((n + MPN_BED_TILE - 1) / MPN_BED_TILE);
    if (u.tmax.alloc((size_t)nb) || u.part.alloc((size_t)2 * nb) || u.total.alloc(2) || u.m_key.alloc((size_t)n) || u.m_start.alloc((size_t)n) ||
        u.m_end.alloc((size_t)n) || u.m_before.alloc((size_t)n)) return -1;
    hipLaunchKernelGGL(bu_tile_max_kernel, dim3(nb), dim3(BU_THREADS), 0, st, (const Rec3 *)rec, n, u.tmax.p);
    hipLaunchKernelGGL(bu_prefix_kernel, dim3(1), dim3(1024), 0, st, u.tmax.p, nb, 1, 1, (uint64_t *)nullptr);
    hipLaunchKernelGGL(bu_count_kernel, dim3(nb), dim3(BU_THREADS), 0, st, (const Rec3 *)rec, n, (const uint64_t *)u.tmax.p, u.part.p, nb);
    hipLaunchKernelGGL(bu_prefix_kernel, dim3(1), dim3(1024), 0, st, u.part.p, nb, 2, 0, u.total.p);
    hipLaunchKernelGGL(bu_fill_kernel, dim3(nb), dim3(BU_THREADS), 0, st, (const Rec3 *)rec, n, (const uint64_t *)u.tmax.p, (const uint64_t *)u.part.p, nb, d_key_group,
                       u.m_key.p, u.m_start.p, u.m_end.p, u.m_before.p, d_span);
    MPN_HIP_CHECK(hipGetLastError());
    // d_hi / d_lo are read by the fill kernel queued above: they must outlive it
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// Checks the n intervals and packs the non-empty ones; returns 0, or -2 with the error set.  skip: the digits no record has --
// the bytes of the start above the largest one, those of the key above n_keys, and all of `end`, which the sweep does not need
// in order.
static int bed_pack(const char *who, int64_t n, const int32_t *key, const int64_t *start, const int64_t *end, int32_t n_keys, std::vector<uint64_t> &hi,
                    std::vector<uint64_t> &lo, uint32_t *skip) {
    int64_t max_start = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (key[i] < 0 || key[i] >= n_keys || start[i] < 0 || start[i] > 0xffffffffLL || end[i] < 0 || end[i] > 0xffffffffLL) {
            set_error("%s: record %lld outside the domain (key in [0, n_keys), 0 <= start, end < 2^32)", who, (long long)i);
            return -2;
        }
        if (start[i] >= end[i]) continue;
        hi.push_back((uint64_t)key[i] + 1);
        lo.push_back((uint64_t)start[i] << 32 | (uint64_t)end[i]);
        max_start = std::max(max_start, start[i]);
    }
    *skip = 0xf;
    for (int p = 0; p < 4; ++p) if (((uint64_t)max_start >> (8 * p)) == 0) *skip |= 1u << (4 + p);
    for (int p = 0; p < 8; ++p) if (((uint64_t)n_keys >> (8 * p)) == 0) *skip |= 1u << (8 + p);
    return 0;
}

// ---- the best alignment of every read: candidates, the abundance-weighted draw, the second best ------------------------------
// (align_list_to_best_align_list and step_unique_alignment of the reference.)  Everything here is a segmented inclusive scan over
// a list ordered by read: element i carries a value and `head` = 1 where its segment starts; join(a, b) = b if b.head, else
// merge(a, b), and head = a.head | b.head -- associative whenever merge is.  A pass P names the value type V, identity(), merge(),
// load(i) and store(i, inclusive value).  Three launches a pass, a lane per element over tiles of MPN_BEST_TILE, like the bu_*
// kernels: the joined value of every tile; one block that turns those into what enters each tile; the rescan that stores.
constexpr int BA_THREADS = 256, BA_ITEMS = MPN_BEST_TILE / BA_THREADS;
static_assert(MPN_BEST_TILE % BA_THREADS == 0, "a tile is whole blocks of lanes");

template <class V>
__device__ __forceinline__ V ba_shfl_up(const V &v, int d) {
    static_assert(sizeof(V) % 4 == 0, "moved lane to lane as 32-bit words");
    int w[sizeof(V) / 4];
    __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
    for (unsigned k = 0; k < sizeof(V) / 4; ++k) w[k] = __shfl_up(w[k], d);
    V o;
    __builtin_memcpy(&o, w, sizeof(V));
    return o;
}

template <class P>
__device__ __forceinline__ typename P::V ba_join(const typename P::V &a, const typename P::V &b) {
    typename P::V r = b.head ? b : P::merge(a, b);
    r.head = a.head | b.head;
    return r;
}

// One step over the block's 256 elements: v -> its inclusive value over the whole list; run: the joined value of everything before
// these 256, moved on to include them.  Every lane of the block calls it (one barrier); ws alternates between steps.
template <class P>
__device__ __forceinline__ typename P::V ba_step(typename P::V v, typename P::V &run, typename P::V *ws) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const typename P::V o = ba_shfl_up(v, d);
        if (lane >= d) v = ba_join<P>(o, v);
    }
    if (lane == 63) ws[wv] = v;
    __syncthreads();
    typename P::V before = run, all = run;
#pragma unroll
    for (int w = 0; w < BA_THREADS / 64; ++w) {
        const typename P::V t = ws[w];
        if (w < wv) before = ba_join<P>(before, t);
        all = ba_join<P>(all, t);
    }
    run = all;
    return ba_join<P>(before, v);
}

// APPLY = false: tiles[tile] = the joined value of the tile.  APPLY = true: tiles[tile] is what enters the tile; store everything.
template <class P, bool APPLY>
__global__ __launch_bounds__(BA_THREADS) void ba_scan_kernel(P p, int64_t n, typename P::V *__restrict__ tiles) {
    __shared__ typename P::V ws[2][BA_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * MPN_BEST_TILE;
    typename P::V run = P::identity();
    if (APPLY) run = tiles[blockIdx.x];
#pragma unroll
    for (int k = 0; k < BA_ITEMS; ++k) {
        if (base + k * BA_THREADS >= n) break;   // (the whole block leaves together)
        const int64_t i = base + k * BA_THREADS + threadIdx.x;
        typename P::V v = P::identity();
        if (i < n) v = p.load(i);
        const typename P::V inc = ba_step<P>(v, run, ws[k & 1]);
        if (APPLY && i < n) p.store(i, inc);
    }
    if (!APPLY && threadIdx.x == 0) tiles[blockIdx.x] = run;
}

// one block, in place: tiles[t] = the joined value of the tiles before t
template <class P>
__global__ __launch_bounds__(BA_THREADS) void ba_carry_kernel(typename P::V *__restrict__ tiles, int nb) {
    __shared__ typename P::V sh[BA_THREADS];
    const int t = threadIdx.x, per = (nb + BA_THREADS - 1) / BA_THREADS, lo = min(nb, t * per), hi = min(nb, lo + per);
    typename P::V s = P::identity();
    for (int k = lo; k < hi; ++k) s = ba_join<P>(s, tiles[k]);
    sh[t] = s;
    __syncthreads();
    if (t == 0) {
        typename P::V acc = P::identity();
        for (int k = 0; k < BA_THREADS; ++k) { const typename P::V v = sh[k]; sh[k] = acc; acc = ba_join<P>(acc, v); }
    }
    __syncthreads();
    typename P::V o = sh[t];
    for (int k = lo; k < hi; ++k) { const typename P::V v = tiles[k]; tiles[k] = o; o = ba_join<P>(o, v); }
}

template <class P>
static int ba_scan(const P &p, int64_t n, hipStream_t st) {
    const int nb = (int)((n + MPN_BEST_TILE - 1) / MPN_BEST_TILE);
    DevBuf<typename P::V> tiles;
    if (tiles.alloc((size_t)nb)) return -1;
    hipLaunchKernelGGL((ba_scan_kernel<P, false>), dim3(nb), dim3(BA_THREADS), 0, st, p, n, tiles.p);
    hipLaunchKernelGGL((ba_carry_kernel<P>), dim3(1), dim3(BA_THREADS), 0, st, tiles.p, nb);
    hipLaunchKernelGGL((ba_scan_kernel<P, true>), dim3(nb), dim3(BA_THREADS), 0, st, p, n, tiles.p);
    MPN_HIP_CHECK(hipGetLastError());
    MPN_HIP_CHECK(hipStreamSynchronize(st));   // `tiles` is read by the kernels queued above: it must outlive them
    return 0;
}

constexpr int64_t BA_MIN = INT64_MIN;   // no score: the domain leaves it out

// the bits of a finite double as an unsigned integer of the same order
static inline uint64_t ba_ordered_bits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u >> 63 ? ~u : u | 0x8000000000000000ULL;
}

// Rows sorted by lo = read << 32 | assembly, input order kept among equal keys.  A segment is one (read, assembly); the scan is the
// arg-max of (score, tiebreak), the later row winning among equal ones.  The last row of a segment then knows the segment's kept
// row: w_idx[i] = that row (-1 on every other i), w_score[i] = its score.
struct BaGroupPass {
    struct V { int64_t score; uint64_t tb; int64_t idx; int32_t head, pad; };
    const Rec3 *rec; const int64_t *score; const uint64_t *tb; int64_t n; int64_t *w_idx, *w_score;
    __device__ static V identity() { return V{BA_MIN, 0, -1, 0, 0}; }
    __device__ static V merge(const V &a, const V &b) { return (b.score > a.score || (b.score == a.score && b.tb >= a.tb)) ? b : a; }
    __device__ V load(int64_t i) const {
        const Rec3 r = rec[i];
        return V{score[r.idx], tb[r.idx], r.idx, i == 0 || rec[i - 1].lo != r.lo, 0};
    }
    __device__ void store(int64_t i, const V &inc) const {
        const bool tail = i + 1 == n || rec[i + 1].lo != rec[i].lo;
        w_idx[i] = tail ? inc.idx : -1;
        w_score[i] = inc.score;
    }
};

// A segment is one read; over its kept rows: the largest score and how many have it.  The last row of a read stores both.
struct BaReadPass {
    struct V { int64_t mx, cnt; int32_t head, pad; };
    const Rec3 *rec; const int64_t *w_idx, *w_score; int64_t n; int64_t *r_max, *r_cnt;
    __device__ static V identity() { return V{BA_MIN, 0, 0, 0}; }
    __device__ static V merge(const V &a, const V &b) { return a.mx > b.mx ? a : b.mx > a.mx ? b : V{a.mx, a.cnt + b.cnt, 0, 0}; }
    __device__ V load(int64_t i) const {
        const bool kept = w_idx[i] >= 0;
        return V{kept ? w_score[i] : BA_MIN, kept ? 1 : 0, i == 0 || (rec[i - 1].lo >> 32) != (rec[i].lo >> 32), 0};
    }
    __device__ void store(int64_t i, const V &inc) const {
        const uint64_t r = rec[i].lo >> 32;
        if (i + 1 == n || (rec[i + 1].lo >> 32) != r) { r_max[r] = inc.mx; r_cnt[r] = inc.cnt; }
    }
};

// No segments: the running count of candidates (kept rows with their read's largest score) puts each into its place in the list.
struct BaCompactPass {
    struct V { int64_t c; int32_t head, pad; };
    const Rec3 *rec; const int64_t *w_idx, *w_score, *r_max; int64_t n; int64_t *cand_row; int32_t *cand_read; int64_t *n_cand;
    __device__ static V identity() { return V{0, 0, 0}; }
    __device__ static V merge(const V &a, const V &b) { return V{a.c + b.c, 0, 0}; }
    __device__ bool candidate(int64_t i) const { return w_idx[i] >= 0 && w_score[i] == r_max[rec[i].lo >> 32]; }
    __device__ V load(int64_t i) const { return V{candidate(i) ? 1 : 0, 0, 0}; }
    __device__ void store(int64_t i, const V &inc) const {
        if (candidate(i)) { cand_row[inc.c - 1] = w_idx[i]; cand_read[inc.c - 1] = (int32_t)(rec[i].lo >> 32); }
        if (i + 1 == n) n_cand[0] = inc.c;
    }
};

// No segments, like BaCompactPass: the running count of GOOD rows -- kept rows whose score reaches `threshold` times their read's
// largest (the reference's good_align_list, bin/megapath_nano.py:642-663) -- puts each into its place in the list.  The bar is one
// IEEE float64 product, formed by __dmul_rn and compared: with no addition beside it there is nothing to contract into an FMA, and
// the intrinsic says so whatever the flags.  Both conversions are exact (|score| < 2^53).
struct BaGoodPass {
    struct V { int64_t c; int32_t head, pad; };
    const Rec3 *rec; const int64_t *w_idx, *w_score, *r_max; int64_t n; int32_t use_threshold; double threshold; int64_t *good_row, *n_good;
    __device__ static V identity() { return V{0, 0, 0}; }
    __device__ static V merge(const V &a, const V &b) { return V{a.c + b.c, 0, 0}; }
    __device__ bool good(int64_t i) const {
        if (w_idx[i] < 0) return false;
        if (!use_threshold) return true;
        const double bar = __dmul_rn((double)r_max[rec[i].lo >> 32], threshold);
        return (double)w_score[i] >= bar;
    }
    __device__ V load(int64_t i) const { return V{good(i) ? 1 : 0, 0, 0}; }
    __device__ void store(int64_t i, const V &inc) const {
        if (good(i)) good_row[inc.c - 1] = w_idx[i];
        if (i + 1 == n) n_good[0] = inc.c;
    }
};

// Rows sorted by lo = key, input order kept among equal keys.  A segment is one key: the number of its rows and the running sums of
// up to BA_SUM_COLS columns (a column the caller did not give is loaded as 0), stored by the key's last row.  64 bytes a value;
// integer addition is exact in any order, so the shape of the scan plays no part in the result.  No atomics: one key may hold most
// of the rows (the assembly that most reads hit), and the scan costs the same whatever the distribution.
constexpr int BA_SUM_COLS = 6;
struct BaSumPass {
    struct V { int64_t cnt; int64_t s[BA_SUM_COLS]; int32_t head, pad; };
    const Rec3 *rec; const int64_t *cols; int64_t n; int32_t n_cols, n_keys; int64_t *count, *sums;
    __device__ static V identity() { V v; v.cnt = 0; for (int c = 0; c < BA_SUM_COLS; ++c) v.s[c] = 0; v.head = 0; v.pad = 0; return v; }
    __device__ static V merge(const V &a, const V &b) {
        V v;
        v.cnt = a.cnt + b.cnt;
#pragma unroll
        for (int c = 0; c < BA_SUM_COLS; ++c) v.s[c] = a.s[c] + b.s[c];
        v.head = 0; v.pad = 0;
        return v;
    }
    __device__ V load(int64_t i) const {
        const Rec3 r = rec[i];
        V v;
        v.cnt = 1;
#pragma unroll
        for (int c = 0; c < BA_SUM_COLS; ++c) v.s[c] = c < n_cols ? cols[(size_t)c * (size_t)n + (size_t)r.idx] : 0;
        v.head = i == 0 || rec[i - 1].lo != r.lo;
        v.pad = 0;
        return v;
    }
    __device__ void store(int64_t i, const V &inc) const {
        const uint64_t k = rec[i].lo;
        if (i + 1 != n && rec[i + 1].lo == k) return;
        count[k] = inc.cnt;
#pragma unroll
        for (int c = 0; c < BA_SUM_COLS; ++c) if (c < n_cols) sums[(size_t)c * (size_t)n_keys + k] = inc.s[c];
    }
};
static_assert(sizeof(BaSumPass::V) == 64, "the count, six sums and head");

// A segment is one read of the candidate list: its summed weight and its number of candidates, stored by its last candidate.
struct BaWeightPass {
    struct V { int64_t sum, cnt; int32_t head, pad; };
    const int32_t *read; const int64_t *weight; int64_t m; int64_t *r_sum, *r_cnt;
    __device__ static V identity() { return V{0, 0, 0, 0}; }
    __device__ static V merge(const V &a, const V &b) { return V{a.sum + b.sum, a.cnt + b.cnt, 0, 0}; }
    __device__ V load(int64_t j) const { return V{weight[j], 1, j == 0 || read[j - 1] != read[j], 0}; }
    __device__ void store(int64_t j, const V &inc) const {
        if (j + 1 == m || read[j + 1] != read[j]) { r_sum[read[j]] = inc.sum; r_cnt[read[j]] = inc.cnt; }
    }
};

// The new tiebreaker of every candidate.  One division and one multiplication in float64, as numpy does them: the file is built
// without fast-math, and a product of a quotient leaves nothing to contract.
__global__ __launch_bounds__(256) void ba_tiebreak_kernel(const int32_t *__restrict__ read, const int64_t *__restrict__ weight, const double *__restrict__ tiebreak,
                                                          const double *__restrict__ draw, int64_t m, const int64_t *__restrict__ r_sum,
                                                          const int64_t *__restrict__ r_cnt, double *__restrict__ out) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = read[j];
        if (r_cnt[r] == 1) { out[j] = tiebreak[j]; continue; }
        const int64_t s = r_sum[r];
        const double relative = s <= 0 ? 1.0 : (double)weight[j] / (double)s;
        out[j] = draw[j] * relative;
    }
}

// A segment is one read of the candidate list: the arg-max of the new tiebreaker, the later candidate winning among equal ones.
struct BaPickPass {
    struct V { double tb; int64_t idx; int32_t head, pad; };
    const int32_t *read; const double *tb; int64_t m; int64_t *winner;
    __device__ static V identity() { return V{-__builtin_huge_val(), -1, 0, 0}; }
    __device__ static V merge(const V &a, const V &b) { return b.tb >= a.tb ? b : a; }
    __device__ V load(int64_t j) const { return V{tb[j], j, j == 0 || read[j - 1] != read[j], 0}; }
    __device__ void store(int64_t j, const V &inc) const {
        if (j + 1 == m || read[j + 1] != read[j]) winner[read[j]] = inc.idx;
    }
};

__global__ __launch_bounds__(256) void ba_fill_kernel(int64_t *__restrict__ out, int64_t n, int64_t value) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = value;
}

// second[r] = max(second[r], score) over the rows of read r off its excluded assembly.  The plain read first: the value only grows,
// so a row that cannot raise it needs no atomic -- a read with many rows would otherwise queue them all on one address.
__global__ __launch_bounds__(256) void ba_second_kernel(const int32_t *__restrict__ read, const int32_t *__restrict__ assembly, const int64_t *__restrict__ score,
                                                        int64_t n, const int32_t *__restrict__ excluded, long long *second) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = read[i];
        if (assembly[i] == excluded[r]) continue;
        const long long s = score[i];
        if (__atomic_load_n(&second[r], __ATOMIC_RELAXED) < s) atomicMax(&second[r], s);
    }
}

static int ba_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 16)); }

// ---- the plan of a read split (include/mpn_reads.h; the gather is in read_split_kernels.hip) -------------------------------------
// Membership pairs sorted by lo = group << 32 | read.  No segments: the running count of DISTINCT pairs puts each into its place
// among the output reads (a pair given twice counts once, as nanosplit's set of files per read has it).
__global__ __launch_bounds__(256) void sp_fill_kernel(const int32_t *__restrict__ read, const int32_t *__restrict__ group, int64_t m, Rec3 *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = Rec3{0, (uint64_t)(uint32_t)group[i] << 32 | (uint32_t)read[i], i};
}

struct SpUniquePass {
    struct V { int64_t c; int32_t head, pad; };
    const Rec3 *rec; const int32_t *len; int64_t m; int32_t *out_read, *u_group, *u_len; int64_t *n_out;
    __device__ static V identity() { return V{0, 0, 0}; }
    __device__ static V merge(const V &a, const V &b) { return V{a.c + b.c, 0, 0}; }
    __device__ bool first(int64_t i) const { return i == 0 || rec[i - 1].lo != rec[i].lo; }
    __device__ V load(int64_t i) const { return V{first(i) ? 1 : 0, 0, 0}; }
    __device__ void store(int64_t i, const V &inc) const {
        if (first(i)) {
            const uint64_t k = rec[i].lo;
            const int32_t r = (int32_t)(uint32_t)k;
            out_read[inc.c - 1] = r; u_group[inc.c - 1] = (int32_t)(k >> 32); u_len[inc.c - 1] = len[r];
        }
        if (i + 1 == m) n_out[0] = inc.c;
    }
};

// Output reads in order; a segment is one group.  The running sum of the lengths gives every read its offset inside its group's
// block; the last read of a group stores the group's bytes; the first one (and the very last read) close the CSR over the groups
// they pass, empty ones included.
struct SpOffsetPass {
    struct V { int64_t sum; int32_t head, pad; };
    const int32_t *u_group, *u_len; int64_t n_out; int32_t n_groups; int64_t *rel, *g_bytes, *group_first;
    __device__ static V identity() { return V{0, 0, 0}; }
    __device__ static V merge(const V &a, const V &b) { return V{a.sum + b.sum, 0, 0}; }
    __device__ V load(int64_t j) const { return V{u_len[j], j == 0 || u_group[j - 1] != u_group[j], 0}; }
    __device__ void store(int64_t j, const V &inc) const {
        const int32_t g = u_group[j];
        rel[j] = inc.sum - u_len[j];
        if (j == 0 || u_group[j - 1] != g)
            for (int32_t k = j == 0 ? 0 : u_group[j - 1] + 1; k <= g; ++k) group_first[k] = j;
        if (j + 1 == n_out || u_group[j + 1] != g) g_bytes[g] = inc.sum;
        if (j + 1 == n_out)
            for (int32_t k = g + 1; k <= n_groups; ++k) group_first[k] = n_out;
    }
};

// one block: group_byte[g] = the sizes of the groups before g, each rounded up to MPN_SPLIT_ALIGN; group_byte[n_groups] = all of them
__global__ __launch_bounds__(1024) void sp_group_byte_kernel(const int64_t *__restrict__ g_bytes, int32_t n_groups, int64_t *__restrict__ group_byte) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x, per = (n_groups + 1023) / 1024, lo = min(n_groups, t * per), hi = min(n_groups, lo + per);
    constexpr int64_t A = MPN_SPLIT_ALIGN;
    int64_t s = 0;
    for (int k = lo; k < hi; ++k) s += (g_bytes[k] + A - 1) / A * A;
    part[t] = s;
    __syncthreads();
    if (t == 0) { int64_t acc = 0; for (int k = 0; k < 1024; ++k) { const int64_t v = part[k]; part[k] = acc; acc += v; } group_byte[n_groups] = acc; }
    __syncthreads();
    int64_t o = part[t];
    for (int k = lo; k < hi; ++k) { group_byte[k] = o; o += (g_bytes[k] + A - 1) / A * A; }
}

__global__ __launch_bounds__(256) void sp_out_off_kernel(const int32_t *__restrict__ u_group, const int64_t *__restrict__ rel, const int64_t *__restrict__ group_byte,
                                                         int64_t n_out, int64_t *__restrict__ out_off) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_out; j += (int64_t)gridDim.x * blockDim.x) out_off[j] = group_byte[u_group[j]] + rel[j];
}

}  // namespace mpn

using namespace mpn;

extern "C" int mpn_sort_order(int64_t n, const uint64_t *hi, const uint64_t *lo, int64_t *order) {
    if (n < 0 || (n > 0 && (!hi || !lo || !order))) { set_error("mpn_sort_order: bad arguments"); return -2; }
    if (n == 0) return 0;
    hipStream_t st = 0;
    DevBuf<uint64_t> d_hi, d_lo;
    DevBuf<Rec3> a, b;
    DevBuf<int64_t> d_order;
    if (d_hi.upload(hi, (size_t)n, st) || d_lo.upload(lo, (size_t)n, st) || a.alloc((size_t)n) || b.alloc((size_t)n) || d_order.alloc((size_t)n)) return -1;
    const int g = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 16));
    hipLaunchKernelGGL(rs_fill_kernel, dim3(g), dim3(256), 0, st, (const uint64_t *)d_hi.p, (const uint64_t *)d_lo.p, n, a.p);
    Rec3 *res = nullptr;
    if (radix_sort_rec3(a.p, b.p, n, &res, st)) return -1;
    hipLaunchKernelGGL(rs_order_kernel, dim3(g), dim3(256), 0, st, (const Rec3 *)res, n, d_order.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (d_order.download(order, (size_t)n, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mpn_cover_by_group(int64_t n, const int32_t *group, const int32_t *seq, const int64_t *start, const int64_t *end,
                                  int32_t n_groups, int64_t *covered) {
    if (n < 0 || n_groups < 0 || (n_groups > 0 && !covered) || (n > 0 && (!group || !seq || !start || !end))) { set_error("mpn_cover_by_group: bad arguments"); return -2; }
    for (int32_t g = 0; g < n_groups; ++g) covered[g] = 0;
    if (n == 0 || n_groups == 0) return 0;
    std::vector<uint64_t> hi((size_t)n), lo((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (group[i] < 0 || group[i] >= n_groups || seq[i] < 0 || start[i] < 0 || end[i] < start[i] || end[i] > 0xffffffffLL) {
            set_error("mpn_cover_by_group: record %lld outside the domain (group in [0, n_groups), seq >= 0, 0 <= start <= end < 2^32)", (long long)i);
            return -2;
        }
        hi[(size_t)i] = (uint64_t)(uint32_t)group[i] << 32 | (uint32_t)seq[i];
        lo[(size_t)i] = (uint64_t)start[i] << 32 | (uint64_t)end[i];
    }
    hipStream_t st = 0;
    DevBuf<uint64_t> d_hi, d_lo;
    DevBuf<Rec3> a, b;
    if (d_hi.upload(hi.data(), (size_t)n, st) || d_lo.upload(lo.data(), (size_t)n, st) || a.alloc((size_t)n) || b.alloc((size_t)n)) return -1;
    const int g = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 16));
    hipLaunchKernelGGL(rs_fill_kernel, dim3(g), dim3(256), 0, st, (const uint64_t *)d_hi.p, (const uint64_t *)d_lo.p, n, a.p);
    Rec3 *res = nullptr;
    if (radix_sort_rec3(a.p, b.p, n, &res, st)) return -1;
    const int n_chunks = (int)std::max<int64_t>(1, std::min<int64_t>(16384, (n + 255) / 256));
    const int64_t chunk = (n + n_chunks - 1) / n_chunks;
    DevBuf<SweepSum> sums;
    DevBuf<uint64_t> ck;
    DevBuf<uint32_t> ce;
    DevBuf<unsigned long long> d_cov;
    if (sums.alloc((size_t)n_chunks) || ck.alloc((size_t)n_chunks) || ce.alloc((size_t)n_chunks) || d_cov.alloc((size_t)n_groups) || d_cov.zero(st)) return -1;
    const int cg = (n_chunks + 255) / 256;
    hipLaunchKernelGGL(cov_phase1_kernel, dim3(cg), dim3(256), 0, st, (const Rec3 *)res, n, chunk, n_chunks, sums.p);
    hipLaunchKernelGGL(cov_phase2_kernel, dim3(1), dim3(64), 0, st, (const SweepSum *)sums.p, n_chunks, ck.p, ce.p);
    hipLaunchKernelGGL(cov_phase3_kernel, dim3(cg), dim3(256), 0, st, (const Rec3 *)res, n, chunk, n_chunks, (const uint64_t *)ck.p, (const uint32_t *)ce.p,
                       d_cov.p, n_groups);
    MPN_HIP_CHECK(hipGetLastError());
    if (d_cov.download((unsigned long long *)covered, (size_t)n_groups, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mpn_depth_by_key(int64_t n, const int32_t *key, const int64_t *start, const int64_t *end, int32_t n_keys, const int64_t *key_len,
                                const int32_t *key_group, int32_t n_groups, const int32_t *depth_lo, const int32_t *depth_hi, int64_t cap,
                                int32_t *row_key, int64_t *row_start, int64_t *row_end, int32_t *row_depth, int64_t *n_rows,
                                int32_t *bed_key, int64_t *bed_start, int64_t *bed_end, int64_t *n_bed, int64_t *span) {
    const int rows_given = !!row_key + !!row_start + !!row_end + !!row_depth + !!n_rows, bed_given = !!bed_key + !!bed_start + !!bed_end + !!n_bed;
    if (n < 0 || n >= ((int64_t)1 << 30) || n_keys < 0 || n_groups < 0 || (rows_given != 0 && rows_given != 5) || (bed_given != 0 && bed_given != 4) ||
        !depth_lo != !depth_hi || (n_keys > 0 && (!key_len || !key_group)) || (n > 0 && (!key || !start || !end))) {
        set_error("mpn_depth_by_key: bad arguments");
        return -2;
    }
    const bool want_rows = rows_given != 0, want_bed = bed_given != 0;
    if ((want_rows || want_bed) && cap < 2 * n) { set_error("mpn_depth_by_key: cap %lld is below 2n = %lld", (long long)cap, (long long)(2 * n)); return -2; }
    int64_t max_len = 0;
    for (int32_t k = 0; k < n_keys; ++k) {
        if (key_len[k] < 0 || key_len[k] > 0xffffffffLL || key_group[k] < 0 || key_group[k] >= n_groups) {
            set_error("mpn_depth_by_key: key %d outside the domain (0 <= key_len < 2^32, key_group in [0, n_groups))", (int)k);
            return -2;
        }
        max_len = std::max(max_len, key_len[k]);
    }
    for (int64_t i = 0; i < n; ++i)
        if (key[i] < 0 || key[i] >= n_keys || start[i] < 0 || start[i] > 0xffffffffLL || end[i] < 0 || end[i] > 0xffffffffLL) {
            set_error("mpn_depth_by_key: record %lld outside the domain (key in [0, n_keys), 0 <= start, end < 2^32)", (long long)i);
            return -2;
        }
    if (n_rows) *n_rows = 0;
    if (n_bed) *n_bed = 0;
    if (span) for (int32_t g = 0; g < n_groups; ++g) span[g] = 0;
    if (n == 0 || !(want_rows || want_bed || span)) return 0;

    hipStream_t st = 0;
    const int64_t m = 2 * n;
    DevBuf<int32_t> d_key, d_group, d_lo, d_hi;
    DevBuf<int64_t> d_start, d_end, d_len;
    DevBuf<Rec3> a, b;
    if (d_key.upload(key, (size_t)n, st) || d_start.upload(start, (size_t)n, st) || d_end.upload(end, (size_t)n, st) || d_len.upload(key_len, (size_t)n_keys, st) ||
        d_group.upload(key_group, (size_t)n_keys, st) || a.alloc((size_t)m) || b.alloc((size_t)m)) return -1;
    if (depth_lo && (d_lo.upload(depth_lo, (size_t)n_groups, st) || d_hi.upload(depth_hi, (size_t)n_groups, st))) return -1;
    const int g = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 16));
    hipLaunchKernelGGL(dp_events_kernel, dim3(g), dim3(256), 0, st, (const int32_t *)d_key.p, (const int64_t *)d_start.p, (const int64_t *)d_end.p, n,
                       (const int64_t *)d_len.p, a.p);
    MPN_HIP_CHECK(hipGetLastError());
    // digits that no event has: the bytes of the position above the longest key, those of the key above n_keys - 1, and idx is no key
    uint32_t skip = 0;
    for (int p = 0; p < 8; ++p) {
        if (((uint64_t)max_len >> (8 * p)) == 0) skip |= 1u << p;
        if (((uint64_t)(n_keys - 1) >> (8 * p)) == 0) skip |= 1u << (8 + p);
    }
    Rec3 *ev = nullptr;
    if (radix_sort_rec3(a.p, b.p, m, &ev, st, skip)) return -1;

    // the points live in the sort's other buffer: 12 bytes a point in the room of 24 bytes an event
    char *room = (char *)(ev == a.p ? b.p : a.p);
    int32_t *pkey = (int32_t *)room, *pdepth = (int32_t *)(room + (size_t)8 * m);
    uint32_t *ppos = (uint32_t *)(room + (size_t)4 * m);
    const int nb = (int)((m + MPN_DEPTH_TILE - 1) / MPN_DEPTH_TILE);
    DevBuf<int32_t> part, total;
    if (part.alloc((size_t)4 * nb) || total.alloc(8)) return -1;
    hipLaunchKernelGGL(dp_point_count_kernel, dim3(nb), dim3(DP_THREADS), 0, st, (const Rec3 *)ev, m, part.p, nb);
    hipLaunchKernelGGL(dp_prefix_kernel, dim3(1), dim3(1024), 0, st, part.p, nb, 2, total.p);
    hipLaunchKernelGGL(dp_point_fill_kernel, dim3(nb), dim3(DP_THREADS), 0, st, (const Rec3 *)ev, m, (const int32_t *)part.p, nb, pkey, ppos, pdepth);
    const int32_t *n_points = total.p + 1, *lo_p = depth_lo ? d_lo.p : nullptr, *hi_p = depth_lo ? d_hi.p : nullptr;
    hipLaunchKernelGGL(dp_row_count_kernel, dim3(nb), dim3(DP_THREADS), 0, st, (const int32_t *)pkey, (const int32_t *)pdepth, n_points, (const int32_t *)d_group.p,
                       lo_p, hi_p, part.p, nb);
    hipLaunchKernelGGL(dp_prefix_kernel, dim3(1), dim3(1024), 0, st, part.p, nb, 4, total.p + 4);
    MPN_HIP_CHECK(hipGetLastError());
    int32_t h_total[8];
    if (total.download(h_total, 8, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    const int64_t nr = (uint32_t)h_total[4], nbed = (uint32_t)h_total[6];
    if (nr != (int64_t)(uint32_t)h_total[5] || nbed != (int64_t)(uint32_t)h_total[7] || nr > m || nbed > m) {
        set_error("mpn_depth_by_key: %lld row starts, %lld row ends, %lld BED starts, %lld BED ends do not pair up", (long long)nr,
                  (long long)(uint32_t)h_total[5], (long long)nbed, (long long)(uint32_t)h_total[7]);
        return -1;
    }
    DevBuf<int32_t> r_key, r_depth, b_key;
    DevBuf<int64_t> r_start, r_end, b_start, b_end;
    DevBuf<unsigned long long> d_span;
    if (want_rows && (r_key.alloc((size_t)nr) || r_depth.alloc((size_t)nr) || r_start.alloc((size_t)nr) || r_end.alloc((size_t)nr))) return -1;
    if (want_bed && (b_key.alloc((size_t)nbed) || b_start.alloc((size_t)nbed) || b_end.alloc((size_t)nbed))) return -1;
    if (span && (d_span.alloc((size_t)n_groups) || d_span.zero(st))) return -1;
    hipLaunchKernelGGL(dp_row_fill_kernel, dim3(nb), dim3(DP_THREADS), 0, st, (const int32_t *)pkey, (const uint32_t *)ppos, (const int32_t *)pdepth, n_points,
                       (const int32_t *)d_group.p, lo_p, hi_p, (const int32_t *)part.p, nb, want_rows ? r_key.p : nullptr, r_start.p, r_end.p, r_depth.p,
                       want_bed ? b_key.p : nullptr, b_start.p, b_end.p, span ? d_span.p : nullptr);
    MPN_HIP_CHECK(hipGetLastError());
    if (want_rows && (r_key.download(row_key, (size_t)nr, st) || r_start.download(row_start, (size_t)nr, st) || r_end.download(row_end, (size_t)nr, st) ||
                      r_depth.download(row_depth, (size_t)nr, st))) return -1;
    if (want_bed && (b_key.download(bed_key, (size_t)nbed, st) || b_start.download(bed_start, (size_t)nbed, st) || b_end.download(bed_end, (size_t)nbed, st))) return -1;
    if (span && d_span.download((unsigned long long *)span, (size_t)n_groups, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (n_rows) *n_rows = nr;
    if (n_bed) *n_bed = nbed;
    return 0;
}

extern "C" int mpn_bed_union(int64_t n, const int32_t *key, const int64_t *start, const int64_t *end, int32_t n_keys, const int32_t *key_group, int32_t n_groups,
                             int64_t cap, int32_t *out_key, int64_t *out_start, int64_t *out_end, int64_t *n_out, int64_t *span) {
    if (n < 0 || n >= ((int64_t)1 << 31) || n_keys < 0 || n_groups < 0 || !out_key || !out_start || !out_end || !n_out || (n_keys > 0 && !key_group) ||
        (n > 0 && (!key || !start || !end))) {
        set_error("mpn_bed_union: bad arguments");
        return -2;
    }
    if (cap < n) { set_error("mpn_bed_union: cap %lld is below n = %lld", (long long)cap, (long long)n); return -2; }
    for (int32_t k = 0; k < n_keys; ++k)
        if (key_group[k] < 0 || key_group[k] >= n_groups) { set_error("mpn_bed_union: key %d outside the domain (key_group in [0, n_groups))", (int)k); return -2; }
    std::vector<uint64_t> hi, lo;
    uint32_t skip = 0;
    if (bed_pack("mpn_bed_union", n, key, start, end, n_keys, hi, lo, &skip)) return -2;
    *n_out = 0;
    if (span) for (int32_t g = 0; g < n_groups; ++g) span[g] = 0;
    if (hi.empty()) return 0;

    hipStream_t st = 0;
    DevBuf<int32_t> d_group;
    DevBuf<unsigned long long> d_span;
    if (d_group.upload(key_group, (size_t)n_keys, st)) return -1;
    if (span && (d_span.alloc((size_t)n_groups) || d_span.zero(st))) return -1;
    BedUnion u;
    if (bed_union_on_device(u, hi, lo, skip, d_group.p, span ? d_span.p : nullptr, st)) return -1;
    uint64_t h_total[2];
    if (u.total.download(h_total, 2, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    const int64_t m = (int64_t)h_total[0];
    if (m < 1 || m > (int64_t)hi.size()) { set_error("mpn_bed_union: %lld merged intervals out of %zu", (long long)m, hi.size()); return -1; }
    std::vector<uint32_t> h_start((size_t)m), h_end((size_t)m);
    if (u.m_key.download(out_key, (size_t)m, st) || u.m_start.download(h_start.data(), (size_t)m, st) || u.m_end.download(h_end.data(), (size_t)m, st)) return -1;
    if (span && d_span.download((unsigned long long *)span, (size_t)n_groups, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    for (int64_t r = 0; r < m; ++r) { out_start[r] = h_start[(size_t)r]; out_end[r] = h_end[(size_t)r]; }
    *n_out = m;
    return 0;
}

extern "C" int mpn_cover_by_bed(int64_t n_bed, const int32_t *bed_key, const int64_t *bed_start, const int64_t *bed_end,
                                int64_t n_q, const int32_t *q_key, const int64_t *q_start, const int64_t *q_end, int32_t n_keys, int64_t *covered) {
    if (n_bed < 0 || n_bed >= ((int64_t)1 << 31) || n_q < 0 || n_keys < 0 || (n_bed > 0 && (!bed_key || !bed_start || !bed_end)) ||
        (n_q > 0 && (!q_key || !q_start || !q_end || !covered))) {
        set_error("mpn_cover_by_bed: bad arguments");
        return -2;
    }
    std::vector<uint64_t> hi, lo;
    uint32_t skip = 0;
    if (bed_pack("mpn_cover_by_bed", n_bed, bed_key, bed_start, bed_end, n_keys, hi, lo, &skip)) return -2;
    for (int64_t i = 0; i < n_q; ++i)
        if (q_key[i] < 0 || q_key[i] >= n_keys || q_start[i] < 0 || q_start[i] > q_end[i] || q_end[i] > 0xffffffffLL) {
            set_error("mpn_cover_by_bed: query %lld outside the domain (key in [0, n_keys), 0 <= start <= end < 2^32)", (long long)i);
            return -2;
        }
    if (n_q == 0) return 0;
    if (hi.empty()) { for (int64_t i = 0; i < n_q; ++i) covered[i] = 0; return 0; }

    hipStream_t st = 0;
    BedUnion u;
    if (bed_union_on_device(u, hi, lo, skip, nullptr, nullptr, st)) return -1;
    DevBuf<int32_t> d_qk;
    DevBuf<int64_t> d_qs, d_qe, d_cov;
    DevBuf<uint32_t> key_off;
    if (d_qk.upload(q_key, (size_t)n_q, st) || d_qs.upload(q_start, (size_t)n_q, st) || d_qe.upload(q_end, (size_t)n_q, st) || d_cov.alloc((size_t)n_q) ||
        key_off.alloc((size_t)n_keys + 1)) return -1;
    hipLaunchKernelGGL(bu_key_offsets_kernel, dim3((n_keys + 256) / 256), dim3(256), 0, st, (const int32_t *)u.m_key.p, (const uint64_t *)u.total.p, n_keys, key_off.p);
    const int g = (int)std::max<int64_t>(1, std::min<int64_t>((n_q + 255) / 256, 256 * 32));
    hipLaunchKernelGGL(bu_cover_kernel, dim3(g), dim3(256), 0, st, (const int32_t *)d_qk.p, (const int64_t *)d_qs.p, (const int64_t *)d_qe.p, n_q,
                       (const uint32_t *)key_off.p, (const uint32_t *)u.m_start.p, (const uint32_t *)u.m_end.p, (const uint64_t *)u.m_before.p, d_cov.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (d_cov.download(covered, (size_t)n_q, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mpn_best_candidates(int64_t n, const int32_t *read, const int32_t *assembly, const int64_t *score, const double *tiebreak, int32_t n_reads,
                                   int32_t n_assemblies, int64_t *cand_row, int32_t *cand_read, int64_t *n_cand, int64_t *read_count, int64_t *read_first) {
    if (n < 0 || n >= ((int64_t)1 << 31) || n_reads < 0 || n_assemblies < 0 || !n_cand || (n_reads > 0 && (!read_count || !read_first)) ||
        (n > 0 && (!read || !assembly || !score || !tiebreak || !cand_row || !cand_read))) {
        set_error("mpn_best_candidates: bad arguments");
        return -2;
    }
    std::vector<uint64_t> hi((size_t)n, 0), lo((size_t)n), tb((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (read[i] < 0 || read[i] >= n_reads || assembly[i] < 0 || assembly[i] >= n_assemblies || score[i] == BA_MIN || !std::isfinite(tiebreak[i])) {
            set_error("mpn_best_candidates: record %lld outside the domain (read in [0, n_reads), assembly in [0, n_assemblies), score > -2^63, finite tiebreak)",
                      (long long)i);
            return -2;
        }
        lo[(size_t)i] = (uint64_t)read[i] << 32 | (uint64_t)assembly[i];
        tb[(size_t)i] = ba_ordered_bits(tiebreak[i] == 0.0 ? 0.0 : tiebreak[i]);
    }
    *n_cand = 0;
    for (int32_t r = 0; r < n_reads; ++r) read_count[r] = read_first[r] = 0;
    if (n == 0) return 0;

    hipStream_t st = 0;
    DevBuf<uint64_t> d_hi, d_lo, d_tb;
    DevBuf<int64_t> d_score, w_idx, w_score, r_max, r_cnt, d_row, d_n;
    DevBuf<int32_t> d_read;
    DevBuf<Rec3> a, b;
    if (d_hi.upload(hi.data(), (size_t)n, st) || d_lo.upload(lo.data(), (size_t)n, st) || d_tb.upload(tb.data(), (size_t)n, st) ||
        d_score.upload(score, (size_t)n, st) || a.alloc((size_t)n) || b.alloc((size_t)n) || w_idx.alloc((size_t)n) || w_score.alloc((size_t)n) ||
        r_max.alloc((size_t)n_reads) || r_cnt.alloc((size_t)n_reads) || r_cnt.zero(st) || d_row.alloc((size_t)n) || d_read.alloc((size_t)n) || d_n.alloc(1)) return -1;
    hipLaunchKernelGGL(rs_fill_kernel, dim3(ba_grid(n)), dim3(256), 0, st, (const uint64_t *)d_hi.p, (const uint64_t *)d_lo.p, n, a.p);
    hipLaunchKernelGGL(ba_fill_kernel, dim3(ba_grid(n_reads)), dim3(256), 0, st, r_max.p, (int64_t)n_reads, BA_MIN);
    MPN_HIP_CHECK(hipGetLastError());
    // digits that no record has: all of hi, the bytes of the assembly above n_assemblies - 1 and those of the read above n_reads - 1
    uint32_t skip = 0xff00;
    for (int p = 0; p < 4; ++p) {
        if (((uint64_t)(n_assemblies - 1) >> (8 * p)) == 0) skip |= 1u << p;
        if (((uint64_t)(n_reads - 1) >> (8 * p)) == 0) skip |= 1u << (4 + p);
    }
    Rec3 *rec = nullptr;
    if (radix_sort_rec3(a.p, b.p, n, &rec, st, skip)) return -1;
    if (ba_scan(BaGroupPass{rec, d_score.p, d_tb.p, n, w_idx.p, w_score.p}, n, st) ||
        ba_scan(BaReadPass{rec, w_idx.p, w_score.p, n, r_max.p, r_cnt.p}, n, st) ||
        ba_scan(BaCompactPass{rec, w_idx.p, w_score.p, r_max.p, n, d_row.p, d_read.p, d_n.p}, n, st)) return -1;
    int64_t m = 0;
    if (d_n.download(&m, 1, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (m < 1 || m > n) { set_error("mpn_best_candidates: %lld candidates out of %lld rows", (long long)m, (long long)n); return -1; }
    if (d_row.download(cand_row, (size_t)m, st) || d_read.download(cand_read, (size_t)m, st) || r_cnt.download(read_count, (size_t)n_reads, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    int64_t first = 0;
    for (int32_t r = 0; r < n_reads; ++r) { read_first[r] = first; first += read_count[r]; }
    if (first != m) { set_error("mpn_best_candidates: the counts per read sum to %lld, the list holds %lld", (long long)first, (long long)m); return -1; }
    *n_cand = m;
    return 0;
}

extern "C" int mpn_pick_weighted(int64_t m, const int32_t *read, const int64_t *weight, const double *tiebreak, const double *draw, int32_t n_reads,
                                 double *new_tiebreak, int64_t *winner) {
    if (m < 0 || m >= ((int64_t)1 << 31) || n_reads < 0 || (n_reads > 0 && !winner) || (m > 0 && (!read || !weight || !tiebreak || !draw || !new_tiebreak))) {
        set_error("mpn_pick_weighted: bad arguments");
        return -2;
    }
    int64_t sum = 0;
    for (int64_t j = 0; j < m; ++j) {
        const bool head = j == 0 || read[j] != read[j - 1];
        if (head) sum = 0;
        if (read[j] < 0 || read[j] >= n_reads || (j > 0 && read[j] < read[j - 1]) || weight[j] < 0 || weight[j] >= ((int64_t)1 << 53) ||
            (sum += weight[j]) >= ((int64_t)1 << 53) || !std::isfinite(tiebreak[j]) || !std::isfinite(draw[j])) {
            set_error("mpn_pick_weighted: candidate %lld outside the domain (read in [0, n_reads) and non-decreasing, weight >= 0 with sums below 2^53 per read, "
                      "finite tiebreak and draw)", (long long)j);
            return -2;
        }
    }
    for (int32_t r = 0; r < n_reads; ++r) winner[r] = -1;
    if (m == 0) return 0;

    hipStream_t st = 0;
    DevBuf<int32_t> d_read;
    DevBuf<int64_t> d_weight, r_sum, r_cnt, d_winner;
    DevBuf<double> d_tb, d_draw, d_out;
    if (d_read.upload(read, (size_t)m, st) || d_weight.upload(weight, (size_t)m, st) || d_tb.upload(tiebreak, (size_t)m, st) || d_draw.upload(draw, (size_t)m, st) ||
        r_sum.alloc((size_t)n_reads) || r_cnt.alloc((size_t)n_reads) || r_sum.zero(st) || r_cnt.zero(st) || d_winner.alloc((size_t)n_reads) || d_out.alloc((size_t)m)) return -1;
    hipLaunchKernelGGL(ba_fill_kernel, dim3(ba_grid(n_reads)), dim3(256), 0, st, d_winner.p, (int64_t)n_reads, (int64_t)-1);
    MPN_HIP_CHECK(hipGetLastError());
    if (ba_scan(BaWeightPass{d_read.p, d_weight.p, m, r_sum.p, r_cnt.p}, m, st)) return -1;
    hipLaunchKernelGGL(ba_tiebreak_kernel, dim3(ba_grid(m)), dim3(256), 0, st, (const int32_t *)d_read.p, (const int64_t *)d_weight.p, (const double *)d_tb.p,
                       (const double *)d_draw.p, m, (const int64_t *)r_sum.p, (const int64_t *)r_cnt.p, d_out.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (ba_scan(BaPickPass{d_read.p, d_out.p, m, d_winner.p}, m, st)) return -1;
    if (d_out.download(new_tiebreak, (size_t)m, st) || d_winner.download(winner, (size_t)n_reads, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mpn_second_best_by_read(int64_t n, const int32_t *read, const int32_t *assembly, const int64_t *score, int32_t n_reads, const int32_t *excluded,
                                       int64_t *second) {
    if (n < 0 || n_reads < 0 || (n_reads > 0 && (!excluded || !second)) || (n > 0 && (!read || !assembly || !score))) {
        set_error("mpn_second_best_by_read: bad arguments");
        return -2;
    }
    for (int64_t i = 0; i < n; ++i)
        if (read[i] < 0 || read[i] >= n_reads || assembly[i] < 0 || score[i] == BA_MIN) {
            set_error("mpn_second_best_by_read: record %lld outside the domain (read in [0, n_reads), assembly >= 0, score > -2^63)", (long long)i);
            return -2;
        }
    for (int32_t r = 0; r < n_reads; ++r)
        if (excluded[r] < -1) { set_error("mpn_second_best_by_read: read %d outside the domain (excluded >= -1)", (int)r); return -2; }
    for (int32_t r = 0; r < n_reads; ++r) second[r] = 0;
    if (n == 0 || n_reads == 0) return 0;

    hipStream_t st = 0;
    DevBuf<int32_t> d_read, d_asm, d_excl;
    DevBuf<int64_t> d_score, d_second;
    if (d_read.upload(read, (size_t)n, st) || d_asm.upload(assembly, (size_t)n, st) || d_score.upload(score, (size_t)n, st) ||
        d_excl.upload(excluded, (size_t)n_reads, st) || d_second.alloc((size_t)n_reads)) return -1;
    hipLaunchKernelGGL(ba_fill_kernel, dim3(ba_grid(n_reads)), dim3(256), 0, st, d_second.p, (int64_t)n_reads, BA_MIN);
    hipLaunchKernelGGL(ba_second_kernel, dim3(ba_grid(n)), dim3(256), 0, st, (const int32_t *)d_read.p, (const int32_t *)d_asm.p, (const int64_t *)d_score.p, n,
                       (const int32_t *)d_excl.p, (long long *)d_second.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (d_second.download(second, (size_t)n_reads, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    for (int32_t r = 0; r < n_reads; ++r) if (second[r] == BA_MIN) second[r] = 0;   // no row off the excluded assembly
    return 0;
}

extern "C" int mpn_good_rows(int64_t n, const int32_t *read, const int32_t *unit, const int64_t *score, const double *tiebreak, int32_t n_reads,
                             int32_t n_units, int32_t use_threshold, double threshold, int64_t *good_row, int64_t *n_good, int64_t *read_best) {
    if (n < 0 || n >= ((int64_t)1 << 31) || n_reads < 0 || n_units < 0 || !n_good || (n_reads > 0 && !read_best) || !std::isfinite(threshold) ||
        (n > 0 && (!read || !unit || !score || !tiebreak || !good_row))) {
        set_error("mpn_good_rows: bad arguments (n in [0, 2^31), n_reads and n_units >= 0, a finite threshold, no NULL array)");
        return -2;
    }
    constexpr int64_t LIMIT = (int64_t)1 << 53;
    std::vector<uint64_t> hi((size_t)n, 0), lo((size_t)n), tb((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (read[i] < 0 || read[i] >= n_reads || unit[i] < 0 || unit[i] >= n_units || score[i] <= -LIMIT || score[i] >= LIMIT || !std::isfinite(tiebreak[i])) {
            set_error("mpn_good_rows: record %lld outside the domain (read in [0, n_reads), unit in [0, n_units), |score| < 2^53, finite tiebreak)", (long long)i);
            return -2;
        }
        lo[(size_t)i] = (uint64_t)read[i] << 32 | (uint64_t)unit[i];
        tb[(size_t)i] = ba_ordered_bits(tiebreak[i] == 0.0 ? 0.0 : tiebreak[i]);
    }
    *n_good = 0;
    for (int32_t r = 0; r < n_reads; ++r) read_best[r] = 0;
    if (n == 0) return 0;

    hipStream_t st = 0;
    DevBuf<uint64_t> d_hi, d_lo, d_tb;
    DevBuf<int64_t> d_score, w_idx, w_score, r_max, r_cnt, d_row, d_n;
    DevBuf<Rec3> a, b;
    if (d_hi.upload(hi.data(), (size_t)n, st) || d_lo.upload(lo.data(), (size_t)n, st) || d_tb.upload(tb.data(), (size_t)n, st) ||
        d_score.upload(score, (size_t)n, st) || a.alloc((size_t)n) || b.alloc((size_t)n) || w_idx.alloc((size_t)n) || w_score.alloc((size_t)n) ||
        r_max.alloc((size_t)n_reads) || r_cnt.alloc((size_t)n_reads) || r_cnt.zero(st) || d_row.alloc((size_t)n) || d_n.alloc(1)) return -1;
    hipLaunchKernelGGL(rs_fill_kernel, dim3(ba_grid(n)), dim3(256), 0, st, (const uint64_t *)d_hi.p, (const uint64_t *)d_lo.p, n, a.p);
    hipLaunchKernelGGL(ba_fill_kernel, dim3(ba_grid(n_reads)), dim3(256), 0, st, r_max.p, (int64_t)n_reads, BA_MIN);
    MPN_HIP_CHECK(hipGetLastError());
    // digits that no record has: all of hi, the bytes of the unit above n_units - 1 and those of the read above n_reads - 1
    uint32_t skip = 0xff00;
    for (int p = 0; p < 4; ++p) {
        if (((uint64_t)(n_units - 1) >> (8 * p)) == 0) skip |= 1u << p;
        if (((uint64_t)(n_reads - 1) >> (8 * p)) == 0) skip |= 1u << (4 + p);
    }
    Rec3 *rec = nullptr;
    if (radix_sort_rec3(a.p, b.p, n, &rec, st, skip)) return -1;
    if (ba_scan(BaGroupPass{rec, d_score.p, d_tb.p, n, w_idx.p, w_score.p}, n, st) ||
        ba_scan(BaReadPass{rec, w_idx.p, w_score.p, n, r_max.p, r_cnt.p}, n, st) ||
        ba_scan(BaGoodPass{rec, w_idx.p, w_score.p, r_max.p, n, use_threshold, threshold, d_row.p, d_n.p}, n, st)) return -1;
    int64_t m = 0;
    if (d_n.download(&m, 1, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (m < 0 || m > n) { set_error("mpn_good_rows: %lld good rows out of %lld rows", (long long)m, (long long)n); return -1; }
    if (d_row.download(good_row, (size_t)m, st) || r_max.download(read_best, (size_t)n_reads, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    for (int32_t r = 0; r < n_reads; ++r) if (read_best[r] == BA_MIN) read_best[r] = 0;   // a read without rows
    *n_good = m;
    return 0;
}

extern "C" int mpn_sum_by_key(int64_t n, const int32_t *key, int32_t n_keys, int32_t n_cols, const int64_t *cols, int64_t *count, int64_t *sums) {
    if (n < 0 || n >= ((int64_t)1 << 31) || n_keys < 0 || n_cols < 1 || n_cols > BA_SUM_COLS || (n_keys > 0 && (!count || !sums)) || (n > 0 && (!key || !cols))) {
        set_error("mpn_sum_by_key: bad arguments (n in [0, 2^31), n_keys >= 0, n_cols in [1, %d], no NULL array)", BA_SUM_COLS);
        return -2;
    }
    constexpr int64_t LIMIT = (int64_t)1 << 32;
    std::vector<uint64_t> hi((size_t)n, 0), lo((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (key[i] < 0 || key[i] >= n_keys) { set_error("mpn_sum_by_key: record %lld outside the domain (key in [0, n_keys))", (long long)i); return -2; }
        lo[(size_t)i] = (uint64_t)key[i];
    }
    for (int32_t c = 0; c < n_cols; ++c)
        for (int64_t i = 0; i < n; ++i) {
            const int64_t v = cols[(size_t)c * (size_t)n + (size_t)i];
            if (v <= -LIMIT || v >= LIMIT) { set_error("mpn_sum_by_key: record %lld outside the domain (|value| < 2^32 in column %d)", (long long)i, (int)c); return -2; }
        }
    for (int32_t k = 0; k < n_keys; ++k) count[k] = 0;
    for (size_t j = 0; j < (size_t)n_cols * (size_t)n_keys; ++j) sums[j] = 0;
    if (n == 0) return 0;

    hipStream_t st = 0;
    DevBuf<uint64_t> d_hi, d_lo;
    DevBuf<int64_t> d_cols, d_count, d_sums;
    DevBuf<Rec3> a, b;
    if (d_hi.upload(hi.data(), (size_t)n, st) || d_lo.upload(lo.data(), (size_t)n, st) || d_cols.upload(cols, (size_t)n_cols * (size_t)n, st) || a.alloc((size_t)n) ||
        b.alloc((size_t)n) || d_count.alloc((size_t)n_keys) || d_count.zero(st) || d_sums.alloc((size_t)n_cols * (size_t)n_keys) || d_sums.zero(st)) return -1;
    hipLaunchKernelGGL(rs_fill_kernel, dim3(ba_grid(n)), dim3(256), 0, st, (const uint64_t *)d_hi.p, (const uint64_t *)d_lo.p, n, a.p);
    MPN_HIP_CHECK(hipGetLastError());
    // digits that no record has: all of hi, the upper half of lo and the bytes of the key above n_keys - 1
    uint32_t skip = 0xfff0;
    for (int p = 0; p < 4; ++p)
        if (((uint64_t)(n_keys - 1) >> (8 * p)) == 0) skip |= 1u << p;
    Rec3 *rec = nullptr;
    if (radix_sort_rec3(a.p, b.p, n, &rec, st, skip)) return -1;
    if (ba_scan(BaSumPass{rec, d_cols.p, n, n_cols, n_keys, d_count.p, d_sums.p}, n, st)) return -1;
    if (d_count.download(count, (size_t)n_keys, st) || d_sums.download(sums, (size_t)n_cols * (size_t)n_keys, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mpn_reads_split_plan(int32_t n, const int32_t *len, int64_t m, const int32_t *mem_read, const int32_t *mem_group, int32_t n_groups,
                                    int64_t out_cap, int64_t *n_out, int32_t *out_read, int64_t *group_first, int64_t *out_off,
                                    int64_t *group_byte, int64_t *out_bytes) {
    tl_split_ns[0] = 0;
    if (n < 0 || m < 0 || m >= ((int64_t)1 << 31) || n_groups < 0 || out_cap < 0 || !n_out || !group_first || !group_byte || !out_bytes || (n > 0 && !len) ||
        (m > 0 && (!mem_read || !mem_group || !out_read || !out_off))) {
        set_error("mpn_reads_split_plan: bad arguments (n, n_groups, out_cap >= 0, m in [0, 2^31), no NULL array that is needed)");
        return -1;
    }
    for (int32_t i = 0; i < n; ++i)
        if (len[i] < 0) { set_error("mpn_reads_split_plan: read %d has the negative length %d", (int)i, (int)len[i]); return -1; }
    for (int64_t i = 0; i < m; ++i)
        if (mem_read[i] < 0 || mem_read[i] >= n || mem_group[i] < 0 || mem_group[i] >= n_groups) {
            set_error("mpn_reads_split_plan: pair %lld = (read %d, group %d) outside [0, %d) x [0, %d)", (long long)i, (int)mem_read[i], (int)mem_group[i], (int)n, (int)n_groups);
            return -1;
        }
    *n_out = 0;
    *out_bytes = MPN_SPLIT_ALIGN;
    for (int32_t g = 0; g <= n_groups; ++g) { group_first[g] = 0; group_byte[g] = 0; }
    if (m == 0) return 0;

    hipStream_t st = 0;
    DevBuf<int32_t> d_len, d_read, d_group, d_out_read, u_group, u_len;
    DevBuf<int64_t> d_n, rel, g_bytes, d_first, d_gbyte, d_off;
    DevBuf<Rec3> a, b;
    if (d_len.upload(len, (size_t)n, st) || d_read.upload(mem_read, (size_t)m, st) || d_group.upload(mem_group, (size_t)m, st) || a.alloc((size_t)m) || b.alloc((size_t)m) ||
        d_out_read.alloc((size_t)m) || u_group.alloc((size_t)m) || u_len.alloc((size_t)m) || d_n.alloc(1) || rel.alloc((size_t)m) || g_bytes.alloc((size_t)n_groups) ||
        g_bytes.zero(st) || d_first.alloc((size_t)n_groups + 1) || d_gbyte.alloc((size_t)n_groups + 1) || d_off.alloc((size_t)m)) return -1;
    DevTimer tm;
    if (tm.start(st)) return -1;
    hipLaunchKernelGGL(sp_fill_kernel, dim3(ba_grid(m)), dim3(256), 0, st, (const int32_t *)d_read.p, (const int32_t *)d_group.p, m, a.p);
    MPN_HIP_CHECK(hipGetLastError());
    // digits that no record has: all of hi, the bytes of the read above n - 1 and those of the group above n_groups - 1
    uint32_t skip = 0xff00;
    for (int p = 0; p < 4; ++p) {
        if (((uint64_t)(n - 1) >> (8 * p)) == 0) skip |= 1u << p;
        if (((uint64_t)(n_groups - 1) >> (8 * p)) == 0) skip |= 1u << (4 + p);
    }
    Rec3 *rec = nullptr;
    if (radix_sort_rec3(a.p, b.p, m, &rec, st, skip)) return -1;
    if (ba_scan(SpUniquePass{rec, d_len.p, m, d_out_read.p, u_group.p, u_len.p, d_n.p}, m, st)) return -1;
    int64_t k = 0;
    if (d_n.download(&k, 1, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (k < 1 || k > m) { set_error("mpn_reads_split_plan: %lld distinct pairs out of %lld", (long long)k, (long long)m); return -1; }
    if (k > out_cap) { set_error("mpn_reads_split_plan: %lld output reads, room for %lld", (long long)k, (long long)out_cap); return -1; }
    if (ba_scan(SpOffsetPass{u_group.p, u_len.p, k, n_groups, rel.p, g_bytes.p, d_first.p}, k, st)) return -1;
    hipLaunchKernelGGL(sp_group_byte_kernel, dim3(1), dim3(1024), 0, st, (const int64_t *)g_bytes.p, n_groups, d_gbyte.p);
    hipLaunchKernelGGL(sp_out_off_kernel, dim3(ba_grid(k)), dim3(256), 0, st, (const int32_t *)u_group.p, (const int64_t *)rel.p, (const int64_t *)d_gbyte.p, k, d_off.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    if (d_out_read.download(out_read, (size_t)k, st) || d_off.download(out_off, (size_t)k, st) || d_first.download(group_first, (size_t)n_groups + 1, st) ||
        d_gbyte.download(group_byte, (size_t)n_groups + 1, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    double ms = 0;
    if (tm.elapsed_ms(&ms)) return -1;
    tl_split_ns[0] = (int64_t)(ms * 1e6);
    *n_out = k;
    *out_bytes = group_byte[n_groups] + MPN_SPLIT_ALIGN;
    return 0;
}
