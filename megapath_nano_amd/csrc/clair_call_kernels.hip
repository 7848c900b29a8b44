// Clair's probabilities decoded into VCF records, behind include/mpn_call.h.  Semantics: output_from / output_with of Clair's
// clair/call_var.py and its pysam look-ups; the arithmetic shared with the host is
// csrc/clair_call_core.h.
//
//   call_indels_kernel    a wave per site over its range of records: 64 records per step, a ballot of those the pile-up takes, a
//                         prefix count for the first 250 and a look at the previous taken lane for the first of a start; then, a
//                         read of the column at a time, the wave walks its operations 64 at a time (tens_wave_ops_k, tensor_wave.h,
//                         with N moving the reference position), the lane whose operation covers the column spells the event
//                         (call_event_at), and the lanes compare it with the distinct events so far, which live in LDS
//                         (256 x 32 bytes and 256 x 50 bases: 21 KB a wave).  Counts are integers; the list is in the order of
//                         first appearance, so the result is the same from run to run.  Plain vector stores to HBM.
//   call_decode_kernel    a wave per site: the 1179 outcome values in LDS (call_value), per round a wave maximum, the first equal
//                         entry of every list by wave minima, the branch of the script, a look-up over the site's events (lanes over
//                         events, a wave maximum of (count, first appearance)); every lane takes the same branch (call_decode over
//                         CallWave).  5 KB of LDS a wave.
//   call_compact_*        the rows of the emitted sites in site order: counts per 256 sites, their running sum, the scatter.
//   call_quantize_kernel  a lane per probability.
#include "mpn_common.h"
#include "clair_call_core.h"
#include "tensor_wave.h"

namespace mpn {

using namespace mpn_call;

static thread_local double tl_call_ms[3] = {0, 0, 0};     // indels, decode, quantize

static_assert(sizeof(mpn_call_read) == 24 && sizeof(mpn_call_event) == 32 && sizeof(mpn_call_row) == 48, "the layouts the Python layer reads");
static_assert(MPN_CALL_ALT1_AT >= 1 + MAXLEN && MPN_CALL_ALT2_AT - MPN_CALL_ALT1_AT >= 1 + 2 * MAXLEN && MPN_CALL_ALLELE_BYTES - MPN_CALL_ALT2_AT >= 1 + 2 * MAXLEN,
              "the alleles fit their places");

// ---- the events ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void call_indels_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_call_read *__restrict__ reads,
                                                         const int32_t *__restrict__ site, const int64_t *__restrict__ begin, const int64_t *__restrict__ end,
                                                         int64_t contig_len, const int64_t *__restrict__ ev_off, mpn_call_event *__restrict__ events,
                                                         uint8_t *__restrict__ bases, int64_t events_cap, int64_t *__restrict__ counts,
                                                         int32_t *__restrict__ bad_read, int32_t *__restrict__ bad_site) {
    __shared__ mpn_call_event s_ev[MPN_CALL_MAX_EVENTS];
    __shared__ uint8_t s_bases[MPN_CALL_MAX_EVENTS * MAXLEN];
    __shared__ CallEvent s_new;
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t position = site[c], col = position - 1, b = begin[c], e = end[c];
    int64_t taken = 0, last_pos = -1;
    bool any = false, overflow = false;
    int32_t rank = 0, n_ev = 0;
    for (int64_t r0 = b; r0 < e; r0 += 64) {
        const int64_t r = r0 + lane;
        mpn_call_read rd{0, 0, 0, 0};
        if (r < e) rd = reads[r];
        const bool tk = r < e && call_taken(rd.pos, rd.rlen, col);
        const unsigned long long vote = __ballot(tk), below = vote & ((1ull << lane) - 1ull);
        const int64_t index = taken + __popcll(below);
        const int prev_lane = below ? 63 - __clzll((long long)below) : -1;
        const int32_t prev_pos = __shfl(rd.pos, prev_lane < 0 ? 0 : prev_lane);
        const bool first = prev_lane >= 0 ? rd.pos != prev_pos : (!any || (int64_t)rd.pos != last_pos);
        const bool kept = tk && (index < MPN_CALL_MAX_DEPTH || first);
        unsigned long long column = __ballot(kept && call_in_column(rd.pos, rd.rlen, col));
        if (vote) {
            last_pos = __shfl(rd.pos, 63 - __clzll((long long)vote));
            any = true;
            taken += __popcll(vote);
        }
        while (column) {                                   // (the same in every lane)
            const int src = __ffsll((long long)column) - 1;
            column &= column - 1ull;
            const int64_t off = __shfl(rd.off, src), rr = r0 + src;
            const int64_t pos = __shfl(rd.pos, src);
            const int32_t my_rank = rank++;
            TensLayout L;
            if (!tens_layout(text, len, off, &L)) { if (lane == 0) atomicMin(bad_read, (int32_t)rr); continue; }
            if (lane == 0) { s_new.kind = -1; s_new.len = 0; s_new.bad = 0; s_new.del_len = 0; s_new.key_len = 0; }
            __syncthreads();
            const bool good = tens_wave_ops_k<true>(text, L, pos, col, col, lane, [&](int32_t k, uint32_t op, int64_t n, int64_t q_r0, int64_t q0) {
                if ((pile_is_match(op) || op == OP_D || op == OP_N) && q_r0 <= col && col < q_r0 + n) call_event_at(text, L, k, op, n, q_r0, q0, col, &s_new);
            });
            __syncthreads();
            if (!good || s_new.bad) { if (lane == 0) atomicMin(bad_read, (int32_t)rr); continue; }
            if (s_new.kind < 0) continue;
            bool hit = false;
            for (int32_t e0 = 0; e0 < n_ev && !hit; e0 += 64) {
                const int32_t i = e0 + lane;
                const bool same = i < n_ev && call_same_event(s_ev[i], s_bases + i * MAXLEN, s_new);
                if (same) ++s_ev[i].count;
                hit = __ballot(same) != 0ull;
            }
            if (!hit) {
                if (n_ev >= MPN_CALL_MAX_EVENTS) overflow = true;
                else {
                    if (lane == 0) {
                        mpn_call_event E;
                        E.kind = s_new.kind; E.len = s_new.len; E.count = 1; E.rank = my_rank; E.bases = 0;
                        E.clip = s_new.kind == MPN_CALL_DELETION ? call_clip(s_new.len, position, contig_len) : s_new.del_len;
                        E.key_len = s_new.kind == MPN_CALL_DELETION ? E.clip : s_new.key_len;
                        s_ev[n_ev] = E;
                    }
                    if (lane < MAXLEN) s_bases[n_ev * MAXLEN + lane] = s_new.kind == MPN_CALL_INSERTION && lane < call_stored(s_new) ? s_new.bases[lane] : 0;
                    ++n_ev;
                }
            }
            __syncthreads();
        }
    }
    if (lane == 0) {
        counts[c] = n_ev;
        if (overflow) atomicMin(bad_site, (int32_t)c);
    }
    if (!events) return;
    const int64_t at0 = ev_off[c];
    for (int32_t i = lane; i < n_ev; i += 64) {
        if (at0 + i >= events_cap) break;
        mpn_call_event E = s_ev[i];
        E.bases = (at0 + i) * MAXLEN;
        events[at0 + i] = E;
    }
    for (int32_t i = lane; i < n_ev * MAXLEN; i += 64)
        if (at0 + i / MAXLEN < events_cap) bases[at0 * MAXLEN + i] = s_bases[i];
}

// ---- the decoding --------------------------------------------------------------------------------------------------------------
struct CallWave {
    int l;
    __device__ __forceinline__ int lane() const { return l; }
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ float max_f(float v) const {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const float u = __shfl_xor(v, d); v = u > v ? u : v; }
        return v;
    }
    __device__ __forceinline__ int min_i(int v) const {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const int u = __shfl_xor(v, d); v = u < v ? u : v; }
        return v;
    }
    __device__ __forceinline__ long long max_ll(long long v) const {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const long long u = __shfl_xor(v, d); v = u > v ? u : v; }
        return v;
    }
    __device__ __forceinline__ int or_i(int v) const { return __ballot(v != 0) != 0ull; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }      // the block is the wave
};

__global__ __launch_bounds__(64) void call_decode_kernel(const int32_t *__restrict__ site, const float *__restrict__ probs, const int32_t *__restrict__ tensors,
                                                         const uint8_t *__restrict__ refs, const int32_t *__restrict__ ref_n, const uint8_t *__restrict__ contig,
                                                         int64_t contig_len, const int64_t *__restrict__ ev_begin, const int64_t *__restrict__ ev_end,
                                                         const mpn_call_event *__restrict__ events, const uint8_t *__restrict__ bases, int32_t options, int32_t *__restrict__ status,
                                                         mpn_call_row *__restrict__ rows, uint8_t *__restrict__ alleles) {
    __shared__ CallWork W;
    __shared__ float s_probs[MPN_CALL_PROBS];
    __shared__ uint8_t s_ref[MPN_CALL_REF];
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    for (int i = lane; i < MPN_CALL_PROBS; i += 64) s_probs[i] = probs[c * MPN_CALL_PROBS + i];
    if (lane < MPN_CALL_REF) s_ref[lane] = refs[c * MPN_CALL_REF + lane];
    __syncthreads();
    const int64_t e0 = ev_begin[c];
    const CallSite S{s_probs, tensors + c * CELLS, s_ref, ref_n[c], contig, contig_len, (int64_t)site[c], events + e0, bases + e0 * MAXLEN,
                     (int32_t)(ev_end[c] - e0), options};
    const CallWave par{lane};
    mpn_call_row row;
    const int st = call_decode(par, S, &W, &row);
    __syncthreads();
    if (lane == 0) {
        status[c] = st;
        if (st == MPN_CALL_EMITTED) { row.site = (int32_t)c; rows[c] = row; }
    }
    if (st == MPN_CALL_EMITTED)
        for (int i = lane; i < MPN_CALL_ALLELE_BYTES; i += 64) {
            const bool used = i < row.ref_len || (i >= MPN_CALL_ALT1_AT && i < MPN_CALL_ALT1_AT + row.alt1_len) ||
                              (i >= MPN_CALL_ALT2_AT && i < MPN_CALL_ALT2_AT + row.alt2_len);
            alleles[c * MPN_CALL_ALLELE_BYTES + i] = used ? W.alleles[i] : 0;
        }
}

constexpr int COMPACT = 256;
__global__ __launch_bounds__(COMPACT) void call_compact_count_kernel(const int32_t *__restrict__ status, int64_t m, int32_t *__restrict__ block_count) {
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * COMPACT + threadIdx.x;
    const unsigned long long vote = __ballot(c < m && status[c] == MPN_CALL_EMITTED);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_n, __popcll(vote));
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = s_n;
}
__global__ __launch_bounds__(64) void call_compact_scan_kernel(int32_t *__restrict__ block_count, int64_t n_blocks, int64_t *__restrict__ total) {
    // the running sum over the blocks, 64 at a time
    int64_t before = 0;
    const int lane = threadIdx.x;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += 64) {
        const int64_t b = b0 + lane;
        const int v = b < n_blocks ? block_count[b] : 0;
        const int incl = wave_scan_add(v);
        if (b < n_blocks) block_count[b] = (int32_t)(before + incl - v);
        before += __shfl(incl, 63);
    }
    if (lane == 0) *total = before;
}
__global__ __launch_bounds__(COMPACT) void call_compact_scatter_kernel(const int32_t *__restrict__ status, int64_t m, const int32_t *__restrict__ block_off,
                                                                       const mpn_call_row *__restrict__ rows, const uint8_t *__restrict__ alleles,
                                                                       mpn_call_row *__restrict__ out_rows, uint8_t *__restrict__ out_alleles) {
    __shared__ int s_wave[COMPACT / 64];
    const int64_t c = (int64_t)blockIdx.x * COMPACT + threadIdx.x;
    const bool emitted = c < m && status[c] == MPN_CALL_EMITTED;
    const unsigned long long vote = __ballot(emitted);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = __popcll(vote);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (!emitted) return;
    const int64_t at = (int64_t)block_off[blockIdx.x] + before + __popcll(vote & ((1ull << lane) - 1ull));
    out_rows[at] = rows[c];
    const uint4 *from = (const uint4 *)(alleles + c * MPN_CALL_ALLELE_BYTES);
    uint4 *to = (uint4 *)(out_alleles + at * MPN_CALL_ALLELE_BYTES);
    for (int i = 0; i < MPN_CALL_ALLELE_BYTES / 16; ++i) to[i] = from[i];
}

__global__ __launch_bounds__(256) void call_quantize_kernel(float *__restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = call_quantize(p[i]);
}

static int call_time(DevTimer &tm, hipStream_t st, double *ms) {
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return tm.elapsed_ms(ms);
}

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_call_last_device_ms(double *indels_ms, double *decode_ms, double *quantize_ms) {
    if (indels_ms) *indels_ms = tl_call_ms[0];
    if (decode_ms) *decode_ms = tl_call_ms[1];
    if (quantize_ms) *quantize_ms = tl_call_ms[2];
}

extern "C" int32_t mpn_call_indels(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_call_read *reads, int64_t m, const int32_t *site,
                                   const int64_t *begin, const int64_t *end, int64_t contig_len, int64_t *counts, const int64_t *ev_off, void *d_events,
                                   void *d_bases, int64_t events_cap, int64_t *bad_read, int64_t *bad_site) {
    tl_call_ms[0] = 0;
    if (n_reads < 0 || n_reads > 0x7ffffff0 || m < 0 || m > 0x7ffffff0 || text_len < 0 || contig_len < 0 || !bad_read || !bad_site || (n_reads > 0 && !reads) ||
        (m > 0 && (!site || !begin || !end || !counts || (n_reads > 0 && !d_text))) || (d_events && (!ev_off || !d_bases || events_cap < 0))) {
        set_error("mpn_call_indels: bad arguments");
        return -2;
    }
    for (int64_t r = 0; r < n_reads; ++r)
        if (reads[r].off < 0 || reads[r].off > text_len - mpn_bamw::BAMW_FIXED || reads[r].rlen < 0 || reads[r].pos < 0) {
            set_error("mpn_call_indels: read %lld does not lie inside the text", (long long)r);
            return -2;
        }
    for (int64_t c = 0; c < m; ++c)
        if (site[c] < 1 || (c > 0 && site[c] <= site[c - 1]) || begin[c] < 0 || end[c] < begin[c] || end[c] > n_reads ||
            (d_events && (ev_off[c] < 0 || counts[c] < 0 || ev_off[c] + counts[c] > events_cap))) {
            set_error("mpn_call_indels: site %lld: the sites are not ascending 1-based positions, or its range does not lie inside the reads or its "
                      "events inside the list", (long long)c);
            return -2;
        }
    *bad_read = -1;
    *bad_site = -1;
    if (m == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_call_read> d_reads;
    DevBuf<int32_t> d_site, d_bad;
    DevBuf<int64_t> d_begin, d_end, d_counts, d_off;
    DevTimer tm;
    const int32_t none[2] = {0x7fffffff, 0x7fffffff};
    if (d_reads.upload(reads, (size_t)n_reads, st) || d_site.upload(site, (size_t)m, st) || d_begin.upload(begin, (size_t)m, st) ||
        d_end.upload(end, (size_t)m, st) || d_counts.alloc((size_t)m) || (d_events ? d_off.upload(ev_off, (size_t)m, st) : 0) || d_bad.upload(none, 2, st) ||
        tm.start(st))
        return -1;
    hipLaunchKernelGGL(call_indels_kernel, dim3((unsigned)m), dim3(64), 0, st, (const uint8_t *)d_text, text_len, (const mpn_call_read *)d_reads.p,
                       (const int32_t *)d_site.p, (const int64_t *)d_begin.p, (const int64_t *)d_end.p, contig_len, (const int64_t *)(d_events ? d_off.p : nullptr),
                       (mpn_call_event *)d_events, (uint8_t *)d_bases, events_cap, d_counts.p, d_bad.p, d_bad.p + 1);
    MPN_HIP_CHECK(hipGetLastError());
    int32_t bad[2] = {none[0], none[1]};
    if (tm.stop(st) || d_counts.download(counts, (size_t)m, st) || d_bad.download(bad, 2, st)) return -1;
    if (call_time(tm, st, &tl_call_ms[0])) return -1;
    if (bad[0] != none[0]) *bad_read = bad[0];
    if (bad[1] != none[1]) *bad_site = bad[1];
    return 0;
}

extern "C" int32_t mpn_call_decode(int64_t m, const int32_t *site, const void *d_probs, const void *d_tensors, const void *d_refs, const int32_t *ref_n,
                                   const void *d_contig, int64_t contig_len, const int64_t *ev_begin, const int64_t *ev_end, const void *d_events,
                                   const void *d_bases, int64_t n_events, int32_t options, int32_t *status, void *d_rows, void *d_alleles, int64_t *n_rows) {
    tl_call_ms[1] = 0;
    if (m < 0 || m > 0x7ffffff0 || contig_len < 0 || (contig_len > 0 && !d_contig) || n_events < 0 || (n_events > 0 && (!d_events || !d_bases)) || !n_rows ||
        (options & ~7) || (m > 0 && (!site || !d_probs || !d_tensors || !d_refs || !ref_n || !ev_begin || !ev_end || !status || !d_rows || !d_alleles))) {
        set_error("mpn_call_decode: bad arguments");
        return -2;
    }
    for (int64_t c = 0; c < m; ++c)
        if (site[c] < 1 || ref_n[c] <= MPN_TENSOR_FLANK || ref_n[c] > MPN_CALL_REF || ev_begin[c] < 0 || ev_end[c] < ev_begin[c] || ev_end[c] > n_events ||
            ev_end[c] - ev_begin[c] > MPN_CALL_MAX_EVENTS) {
            set_error("mpn_call_decode: site %lld: not a 1-based position, a reference string without a centre, or events that are not a list",
                      (long long)c);
            return -2;
        }
    *n_rows = 0;
    if (m == 0) return 0;
    hipStream_t st = 0;
    const int64_t n_blocks = (m + COMPACT - 1) / COMPACT;
    DevBuf<int32_t> d_site, d_ref_n, d_status, d_block;
    DevBuf<int64_t> d_begin, d_end, d_total;
    DevBuf<mpn_call_row> d_all;
    DevBuf<uint8_t> d_all_alleles;
    DevTimer tm;
    if (d_site.upload(site, (size_t)m, st) || d_ref_n.upload(ref_n, (size_t)m, st) || d_begin.upload(ev_begin, (size_t)m, st) || d_end.upload(ev_end, (size_t)m, st) || d_status.alloc((size_t)m) ||
        d_block.alloc((size_t)n_blocks) || d_total.alloc(1) || d_all.alloc((size_t)m) || d_all_alleles.alloc((size_t)m * MPN_CALL_ALLELE_BYTES) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(call_decode_kernel, dim3((unsigned)m), dim3(64), 0, st, (const int32_t *)d_site.p, (const float *)d_probs, (const int32_t *)d_tensors,
                       (const uint8_t *)d_refs, (const int32_t *)d_ref_n.p, (const uint8_t *)d_contig, contig_len, (const int64_t *)d_begin.p,
                       (const int64_t *)d_end.p, (const mpn_call_event *)d_events, (const uint8_t *)d_bases, options, d_status.p, d_all.p, d_all_alleles.p);
    MPN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(call_compact_count_kernel, dim3((unsigned)n_blocks), dim3(COMPACT), 0, st, (const int32_t *)d_status.p, m, d_block.p);
    MPN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(call_compact_scan_kernel, dim3(1), dim3(64), 0, st, d_block.p, n_blocks, d_total.p);
    MPN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(call_compact_scatter_kernel, dim3((unsigned)n_blocks), dim3(COMPACT), 0, st, (const int32_t *)d_status.p, m, (const int32_t *)d_block.p,
                       (const mpn_call_row *)d_all.p, (const uint8_t *)d_all_alleles.p, (mpn_call_row *)d_rows, (uint8_t *)d_alleles);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st) || d_status.download(status, (size_t)m, st) || d_total.download(n_rows, 1, st)) return -1;
    return call_time(tm, st, &tl_call_ms[1]);
}

extern "C" int32_t mpn_call_quantize(void *d_probs, int64_t n) {
    tl_call_ms[2] = 0;
    if (n < 0 || (n > 0 && !d_probs)) {
        set_error("mpn_call_quantize: bad arguments");
        return -2;
    }
    if (n == 0) return 0;
    hipStream_t st = 0;
    DevTimer tm;
    if (tm.start(st)) return -1;
    hipLaunchKernelGGL(call_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (float *)d_probs, n);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    return call_time(tm, st, &tl_call_ms[2]);
}
