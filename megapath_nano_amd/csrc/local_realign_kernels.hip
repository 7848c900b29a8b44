// Local realignment around called variants on a resident BAM text, behind include/mpn_local_realign.h.  Semantics: the reference's
// realignment/local_realignment.py -p ont; the arithmetic shared with the host is
// csrc/local_realign_core.h.
//
//   lr_cover_kernel     a wave per (site, read) pair: tens_wave_ops_k gives every lane one CIGAR operation, 64 a step, and skips the
//                       steps before the region; a lane ORs what its operation covers into the site's 401 bits (lr_cover_op).
//   lr_hazard_kernel    a wave per place where the script's parser may raise (rare): does an earlier read give it an entry there?
//   lr_mask_kernel      a thread per site: covered and not bad, cut at the first missing column behind the centre.
//   lr_frag_kernel      a wave per pair, twice: the lanes count what their operation appends (lr_frag_op), a wave scan places it
//                       behind what the operations before it gave; the second pass writes the letters and their SSW codes.  Plain
//                       vector stores.
//   lr_refs_kernel      the SSW codes of every site's reference window.
//   (SSW)               ssw_resident (csrc/ssw_kernels.hip) on the codes where they lie.
//   lr_keys_kernel      a thread per pair: the walk over the SSW CIGAR (lr_pair_keys).
//   lr_site_kernel      a wave per site: the distinct keys of its reads, compared 64 table entries at a time; count, first
//                       insertion (the smallest (reference position, place in the dict, place in the walk) of a key) and depth.
//   lr_emit_kernel      a wave per site: the keys in the order of first insertion, their text to the byte arena.
// Integer arithmetic throughout: the results do not depend on the order in which waves run.
#include "mpn_common.h"
#include "local_realign_core.h"
#include "tensor_wave.h"
#include "ssw_resident.h"
#include "../../include/mpn_ssw.h"

namespace mpn {

using namespace mpn_lr;

static thread_local double tl_lr_ms[4] = {0, 0, 0, 0};     // columns, fragments, ssw, tally

static_assert(sizeof(mpn_lr_read) == 16 && sizeof(mpn_lr_pair) == 8 && sizeof(mpn_lr_key) == 16 && sizeof(LrKeyRef) == 16, "the layouts the Python layer reads");

constexpr int LR_THREADS = 256, LR_WAVES = LR_THREADS / 64;
constexpr unsigned long long LR_NONE = ~0ull;

__device__ __forceinline__ void lr_refuse(unsigned long long *bad, int64_t pair, int why) {
    atomicMin(bad, ((unsigned long long)pair << 8) | (unsigned)why);
}

// the reason of the lane with the smallest operation index that has one; 0: none
__device__ __forceinline__ int lr_first_reason(int st, int32_t k) {
    const int v = st ? (int)(((uint32_t)k << 4) | (uint32_t)st) : 0x7fffffff;
    const int w = wave_reduce_min(v);
    return w == 0x7fffffff ? 0 : (w & 15);
}

struct LrAtomicOr {
    uint32_t *cov, *bad;
    __device__ __forceinline__ void operator()(int word, uint32_t c, uint32_t b) {
        if (c) atomicOr(&cov[word], c);
        if (b) atomicOr(&bad[word], b);
    }
};

// what a wave needs of its pair; false (the pair is refused) if it does not exist
struct LrJob { mpn_lr_read rd; TensLayout L; int64_t pos1; int32_t site; };
__device__ __forceinline__ bool lr_job(const uint8_t *__restrict__ text, int64_t len, const mpn_lr_read *__restrict__ reads, int64_t n_reads,
                                       const int32_t *__restrict__ site_pos, int64_t m, const mpn_lr_pair *__restrict__ pairs, int64_t i, int lane,
                                       unsigned long long *bad, LrJob *J) {
    const mpn_lr_pair p = pairs[i];
    int why = 0;
    if (p.site < 0 || p.site >= m || p.read < 0 || p.read >= n_reads) why = MPN_LR_PAST;
    else {
        J->rd = reads[p.read];
        J->site = p.site;
        J->pos1 = site_pos[p.site];
        if (!tens_layout(text, len, J->rd.off, &J->L)) why = MPN_LR_PAST;
        else if (J->L.l_seq == 0) why = MPN_LR_NO_BASES;
    }
    if (why && lane == 0) lr_refuse(bad, i, why);
    return why == 0;
}

__global__ __launch_bounds__(LR_THREADS) void lr_cover_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_lr_read *__restrict__ reads,
                                                              int64_t n_reads, const int32_t *__restrict__ site_pos, int64_t m,
                                                              const mpn_lr_pair *__restrict__ pairs, int64_t n_pairs, uint32_t *cov, uint32_t *badcol,
                                                              unsigned long long *bad, int64_t *hazards, int64_t hazard_cap,
                                                              unsigned long long *n_hazards) {
    const int64_t i = (int64_t)blockIdx.x * LR_WAVES + (threadIdx.x >> 6);
    if (i >= n_pairs) return;                                  // (the whole wave)
    const int lane = threadIdx.x & 63;
    LrJob J;
    if (!lr_job(text, len, reads, n_reads, site_pos, m, pairs, i, lane, bad, &J)) return;
    LrAtomicOr orr{cov + (int64_t)J.site * WORDS, badcol + (int64_t)J.site * WORDS};
    int st = 0;
    int32_t at = 0;
    const bool good = tens_wave_ops_k<true>(text, J.L, J.rd.pos, J.pos1 - REGION - 1, J.pos1 + REGION + 1, lane,
                                            [&](int32_t k, uint32_t op, int64_t n, int64_t r0, int64_t q0) {
        if (k >= J.L.n_cigar || st) return;
        const int s = lr_skip_or_pad(op, n, r0, J.pos1) ? MPN_LR_SKIP_PAD : lr_cover_op(text, J.L, op, n, r0, q0, lr_w0(J.pos1), orr);
        if (s) { st = s; at = k; return; }
        const int64_t hz = lr_hazard_op(text, J.L, k, op, n, r0, q0, J.pos1);
        if (hz >= 0) {                                         // (rare: a slot per hazard, any order)
            const unsigned long long slot = atomicAdd(n_hazards, 1ull);
            if (slot < (unsigned long long)hazard_cap) { hazards[3 * slot] = i; hazards[3 * slot + 1] = hz; hazards[3 * slot + 2] = 0; }
        }
    });
    int why = lr_first_reason(st, at);
    if (!good) why = MPN_LR_BAD_OP;                            // (the walk hands such an operation on as an empty pad)
    if (why && lane == 0) lr_refuse(bad, i, why);
}

// a wave per hazard: does an earlier pair of the site give the parser an entry at the column?  64 earlier pairs a step.
__global__ __launch_bounds__(64) void lr_hazard_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_lr_read *__restrict__ reads,
                                                       const mpn_lr_pair *__restrict__ pairs, int64_t *__restrict__ hazards) {
    const int64_t p = hazards[3 * (int64_t)blockIdx.x], c = hazards[3 * (int64_t)blockIdx.x + 1];
    const int32_t site = pairs[p].site;
    bool covered = false;
    for (int64_t j0 = p - 1; j0 >= 0 && !covered; j0 -= 64) {
        const int64_t j = j0 - threadIdx.x;
        const bool mine = j >= 0 && pairs[j].site == site;
        const bool entry = mine && lr_entry_at(text, len, reads[pairs[j].read].off, reads[pairs[j].read].pos, c);
        covered = __ballot(entry) != 0ull;
        if (__ballot(mine) != ~0ull) break;                    // (the site's first pair lies in this step)
    }
    if (threadIdx.x == 0) hazards[3 * (int64_t)blockIdx.x + 2] = covered ? 0 : 1;
}

__global__ __launch_bounds__(256) void lr_mask_kernel(const uint32_t *__restrict__ cov, const uint32_t *__restrict__ badcol, int64_t m,
                                                      uint32_t *__restrict__ mask) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= m) return;
    uint32_t a[WORDS], b[WORDS], o[WORDS];
    for (int w = 0; w < WORDS; ++w) { a[w] = cov[c * WORDS + w]; b[w] = badcol[c * WORDS + w]; }
    lr_finish_mask(a, b, o);
    for (int w = 0; w < WORDS; ++w) mask[c * WORDS + w] = o[w];
}

struct LrCount {
    int n;
    int64_t first;
    __device__ __forceinline__ void operator()(uint8_t, int64_t col) {
        if (n == 0) first = col;
        ++n;
    }
};
struct LrWrite {
    uint8_t *letters;
    int8_t *codes;
    int64_t at, end;           // where the next byte goes; the end of the pair's fragment
    __device__ __forceinline__ void operator()(uint8_t letter, int64_t) {
        if (at < end) { letters[at] = letter; codes[at] = lr_ssw_code(letter); }
        ++at;
    }
};

template <bool FILL>
__global__ __launch_bounds__(LR_THREADS) void lr_frag_kernel(const uint8_t *__restrict__ text, int64_t len, const mpn_lr_read *__restrict__ reads,
                                                             int64_t n_reads, const int32_t *__restrict__ site_pos, int64_t m,
                                                             const mpn_lr_pair *__restrict__ pairs, int64_t n_pairs, const uint32_t *__restrict__ mask,
                                                             int32_t *__restrict__ frag_len, int32_t *__restrict__ first, const int64_t *__restrict__ frag_off,
                                                             uint8_t *__restrict__ letters, int8_t *__restrict__ codes, int64_t cap, unsigned long long *bad) {
    const int64_t i = (int64_t)blockIdx.x * LR_WAVES + (threadIdx.x >> 6);
    if (i >= n_pairs) return;                                  // (the whole wave)
    const int lane = threadIdx.x & 63;
    int64_t off = 0, end = 0;
    if (FILL) {
        off = frag_off[i];
        if (off < 0) return;
        end = off + frag_len[i];
        if (end > cap) end = cap;
    }
    LrJob J;
    if (!lr_job(text, len, reads, n_reads, site_pos, m, pairs, i, lane, bad, &J)) {
        if (!FILL && lane == 0) { frag_len[i] = 0; first[i] = 0; }
        return;
    }
    const uint32_t *__restrict__ msk = mask + (int64_t)J.site * WORDS;
    const int64_t w0 = lr_w0(J.pos1);
    int st = 0, base = 0;
    int32_t at = 0;
    int64_t head = INT64_MAX;
    const bool good = tens_wave_ops_k<true>(text, J.L, J.rd.pos, J.pos1 - REGION - 1, J.pos1 + REGION + 1, lane,
                                            [&](int32_t k, uint32_t op, int64_t n, int64_t r0, int64_t q0) {
        LrCount cnt{0, 0};
        if (k < J.L.n_cigar && !st) {
            const int s = lr_skip_or_pad(op, n, r0, J.pos1) ? MPN_LR_SKIP_PAD : lr_frag_op(text, J.L, k, op, n, r0, q0, w0, msk, cnt);
            if (s) { st = s; at = k; cnt.n = 0; }
        }
        if (cnt.n && cnt.first < head) head = cnt.first;
        const int incl = wave_scan_add(cnt.n);
        if (FILL && cnt.n) {
            LrWrite wr{letters, codes, off + base + incl - cnt.n, end};
            lr_frag_op(text, J.L, k, op, n, r0, q0, w0, msk, wr);
        }
        base += __builtin_amdgcn_readlane(incl, 63);
    });
    int why = lr_first_reason(st, at);
    if (!good) why = MPN_LR_BAD_OP;                            // (the walk hands such an operation on as an empty pad)
    if (why && lane == 0) lr_refuse(bad, i, why);
    if (!FILL) {
        // the first column over the lanes: 64-bit minimum by two 32-bit ones (columns are below 2^31)
        const int h = wave_reduce_min(head == INT64_MAX ? 0x7fffffff : (int)head);
        if (lane == 0) { frag_len[i] = why ? 0 : base; first[i] = h == 0x7fffffff ? 0 : h; }
    }
}

__global__ __launch_bounds__(256) void lr_refs_kernel(const uint8_t *__restrict__ contig, int64_t contig_len, const int32_t *__restrict__ site_pos, int64_t m,
                                                      int8_t *__restrict__ refs) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= m * MPN_LR_REF_STRIDE) return;
    const int64_t c = g / MPN_LR_REF_STRIDE, j = g - c * MPN_LR_REF_STRIDE;
    const int64_t at = (int64_t)site_pos[c] - FLANK_REF - 1 + j;
    refs[g] = (j <= 2 * FLANK_REF && at >= 0 && at < contig_len) ? lr_ssw_code(contig[at]) : (int8_t)4;
}

// ---- alleles ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lr_keys_kernel(int64_t n_pairs, const int32_t *__restrict__ res, const uint32_t *__restrict__ cig,
                                                      const int64_t *__restrict__ cig_end, const int32_t *__restrict__ cig_len,
                                                      const int64_t *__restrict__ frag_off, const int32_t *__restrict__ frag_len,
                                                      const int32_t *__restrict__ pair_site, const int32_t *__restrict__ site_pos, int64_t contig_len,
                                                      LrKeyRef *__restrict__ keys, int32_t *__restrict__ n_keys, int32_t *__restrict__ ref_pos,
                                                      unsigned long long *bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    const int32_t score = res[i], status = res[7 * n_pairs + i];
    int nk = 0;
    int64_t rp = 0;
    if (status == MPN_SSW_EDOMAIN || status == MPN_SSW_ETOOLONG) lr_refuse(bad, i, status);      // (refused before the launch: the row is zero)
    else if (score > 0) {
        if (status != MPN_SSW_OK) lr_refuse(bad, i, status);
        else {
            const int32_t cl = cig_len[i];
            nk = lr_pair_keys(res[2 * n_pairs + i], res[4 * n_pairs + i], res[5 * n_pairs + i], cig + (cig_end[i] - cl), cl, frag_off[i], frag_len[i],
                              (int64_t)site_pos[pair_site[i]], contig_len, keys + i * MAX_KEYS, &rp);
        }
    }
    n_keys[i] = nk;
    ref_pos[i] = (int32_t)rp;
}

struct LrTable { int32_t *rep, *cnt; unsigned long long *rank; };

__global__ __launch_bounds__(64) void lr_site_kernel(int64_t m, const int64_t *__restrict__ pair_begin, const int32_t *__restrict__ res,
                                                     const LrKeyRef *keys, const int32_t *__restrict__ n_keys, const int32_t *__restrict__ ref_pos,
                                                     const uint8_t *__restrict__ letters, const uint8_t *__restrict__ contig, LrTable tab,
                                                     int32_t *__restrict__ site_keys, int64_t *__restrict__ site_bytes, int32_t *__restrict__ depth,
                                                     int32_t *__restrict__ raises) {
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t b = pair_begin[c], e = pair_begin[c + 1];
    const bool rz = e > b && res[b] <= 0;              // the script's ref_pos is not bound yet: it raises
    int32_t *rep = tab.rep + b * MAX_KEYS, *cnt = tab.cnt + b * MAX_KEYS;
    unsigned long long *rank = tab.rank + b * MAX_KEYS;
    int K = 0;
    for (int64_t j = b; j < e && !rz; ++j) {
        const int nk = n_keys[j];
        for (int s = 0; s < nk; ++s) {
            const LrKeyRef key = keys[j * MAX_KEYS + s];
            const unsigned long long rk = ((unsigned long long)(uint32_t)ref_pos[j] << 32) | ((unsigned long long)(j - b) << 3) | (unsigned)s;
            int found = -1;
            for (int e0 = 0; e0 < K && found < 0; e0 += 64) {
                const int idx = e0 + lane;
                const bool eq = idx < K && lr_key_equal(key, keys[rep[idx]], letters, contig);
                const unsigned long long vote = __ballot(eq);
                if (vote) found = e0 + __ffsll((long long)vote) - 1;
            }
            if (lane == 0) {
                if (found >= 0) {
                    ++cnt[found];
                    if (rk < rank[found]) rank[found] = rk;
                } else {
                    rep[K] = (int32_t)(j * MAX_KEYS + s);
                    cnt[K] = 1;
                    rank[K] = rk;
                }
            }
            if (found < 0) ++K;
            __syncthreads();                           // the table written by lane 0 is read by all lanes in the next round
        }
    }
    int d = 0, bytes = 0;
    for (int idx = lane; idx < K; idx += 64) {
        const LrKeyRef key = keys[rep[idx]];
        const uint8_t c0 = lr_key_char(key, 0, letters, contig);
        if (c0 != 'I' && c0 != 'D') d += cnt[idx];
        bytes += lr_key_strlen(key);
    }
    d = __builtin_amdgcn_readlane(wave_scan_add(d), 63);
    bytes = __builtin_amdgcn_readlane(wave_scan_add(bytes), 63);
    if (lane == 0) { site_keys[c] = K; site_bytes[c] = bytes; depth[c] = d; raises[c] = rz ? 1 : 0; }
}

__global__ __launch_bounds__(64) void lr_emit_kernel(int64_t m, const int64_t *__restrict__ pair_begin, const LrKeyRef *__restrict__ keys,
                                                     const uint8_t *__restrict__ letters, const uint8_t *__restrict__ contig, LrTable tab,
                                                     const int32_t *__restrict__ site_keys, const int64_t *__restrict__ key_begin,
                                                     const int64_t *__restrict__ byte_begin, mpn_lr_key *__restrict__ out, int64_t keys_cap,
                                                     uint8_t *__restrict__ bytes, int64_t bytes_cap) {
    const int64_t c = blockIdx.x;
    const int64_t b = pair_begin[c];
    const int32_t *rep = tab.rep + b * MAX_KEYS, *cnt = tab.cnt + b * MAX_KEYS;
    const unsigned long long *rank = tab.rank + b * MAX_KEYS;
    const int K = site_keys[c];
    for (int idx = threadIdx.x; idx < K; idx += 64) {
        const unsigned long long mine = rank[idx];
        int64_t place = 0, before = 0;
        for (int t = 0; t < K; ++t)
            if (rank[t] < mine) { ++place; before += lr_key_strlen(keys[rep[t]]); }
        const LrKeyRef key = keys[rep[idx]];
        const int32_t n = lr_key_strlen(key);
        const int64_t at = key_begin[c] + place, off = byte_begin[c] + before;
        if (at >= keys_cap || off + n > bytes_cap) continue;   // (the host has sized both)
        out[at] = mpn_lr_key{cnt[idx], n, off};
        for (int32_t k = 0; k < n; ++k) bytes[off + k] = lr_key_char(key, k, letters, contig);
    }
}

static int lr_time(DevTimer &tm, hipStream_t st, double *ms) {
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return tm.elapsed_ms(ms);
}

static bool lr_reads_inside(const mpn_lr_read *reads, int64_t n, int64_t text_len) {
    for (int64_t r = 0; r < n; ++r)
        if (reads[r].off < 0 || reads[r].off > text_len - mpn_bamw::BAMW_FIXED) return false;
    return true;
}

static void lr_bad_out(unsigned long long bad, int64_t *bad_pair, int32_t *bad_why) {
    *bad_pair = bad == LR_NONE ? -1 : (int64_t)(bad >> 8);
    *bad_why = bad == LR_NONE ? 0 : (int32_t)(bad & 255);
}

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_lr_last_device_ms(double *columns_ms, double *fragments_ms, double *ssw_ms, double *tally_ms) {
    if (columns_ms) *columns_ms = tl_lr_ms[0];
    if (fragments_ms) *fragments_ms = tl_lr_ms[1];
    if (ssw_ms) *ssw_ms = tl_lr_ms[2];
    if (tally_ms) *tally_ms = tl_lr_ms[3];
}

extern "C" int32_t mpn_lr_depth_rule(int64_t n, const int64_t *start, const int64_t *end, int32_t maxcnt, uint8_t *keep) {
    if (n < 0 || maxcnt < 0 || (n > 0 && (!start || !end || !keep))) {
        set_error("mpn_lr_depth_rule: bad arguments");
        return -2;
    }
    for (int64_t i = 1; i < n; ++i)
        if (start[i] < start[i - 1]) {
            set_error("mpn_lr_depth_rule: the candidates are not sorted by start");
            return -2;
        }
    lr_depth_rule(n, start, end, maxcnt, keep);
    return 0;
}

static bool lr_common_args(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_lr_read *reads, int64_t m, const int32_t *site_pos,
                           int64_t n_pairs, const mpn_lr_pair *pairs) {
    if (text_len < 0 || n_reads < 0 || n_reads > 0x7ffffff0 || m < 0 || m > 0x7ffffff0 || n_pairs < 0 || n_pairs > 0x7ffffff0 ||
        (n_pairs > 0 && (!d_text || !reads || !site_pos || !pairs)) || (m > 0 && !site_pos) || (n_reads > 0 && !reads) || !lr_reads_inside(reads, n_reads, text_len))
        return false;
    for (int64_t c = 0; c < m; ++c)
        if (site_pos[c] <= MPN_LR_FLANK || site_pos[c] > 0x7ffff000) return false;
    for (int64_t i = 0; i < n_pairs; ++i)
        if (pairs[i].site < 0 || pairs[i].site >= m || pairs[i].read < 0 || pairs[i].read >= n_reads) return false;
    return true;
}

extern "C" int32_t mpn_lr_columns(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_lr_read *reads, int64_t m, const int32_t *site_pos,
                                  int64_t n_pairs, const mpn_lr_pair *pairs, void *d_mask, int64_t *bad_pair, int32_t *bad_why, int64_t *hazards,
                                  int64_t hazard_cap, int64_t *n_hazards) {
    tl_lr_ms[0] = 0;
    if (!bad_pair || !bad_why || !n_hazards || hazard_cap < 0 || (hazard_cap > 0 && !hazards) || (m > 0 && !d_mask) || !lr_common_args(d_text, text_len, n_reads, reads, m, site_pos, n_pairs, pairs)) {
        set_error("mpn_lr_columns: bad arguments, a read that does not lie inside the text, a site at or before position 300, or a pair without its site or read");
        return -2;
    }
    *bad_pair = -1; *bad_why = 0; *n_hazards = 0;
    if (m == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_lr_read> d_reads;
    DevBuf<mpn_lr_pair> d_pairs;
    DevBuf<int32_t> d_pos;
    DevBuf<uint32_t> d_cov, d_badcol;
    DevBuf<unsigned long long> d_bad, d_nhz;
    DevBuf<int64_t> d_hz;
    DevTimer tm;
    if (d_reads.upload(reads, (size_t)n_reads, st) || d_pairs.upload(pairs, (size_t)n_pairs, st) || d_pos.upload(site_pos, (size_t)m, st) ||
        d_cov.alloc((size_t)m * WORDS) || d_badcol.alloc((size_t)m * WORDS) || d_cov.zero(st) || d_badcol.zero(st) || d_bad.upload(&LR_NONE, 1, st) ||
        d_nhz.alloc(1) || d_nhz.zero(st) || d_hz.alloc((size_t)hazard_cap * 3) || tm.start(st))
        return -1;
    if (n_pairs > 0) {
        hipLaunchKernelGGL(lr_cover_kernel, dim3((unsigned)((n_pairs + LR_WAVES - 1) / LR_WAVES)), dim3(LR_THREADS), 0, st, (const uint8_t *)d_text, text_len,
                           (const mpn_lr_read *)d_reads.p, n_reads, (const int32_t *)d_pos.p, m, (const mpn_lr_pair *)d_pairs.p, n_pairs, d_cov.p,
                           d_badcol.p, d_bad.p, d_hz.p, hazard_cap, d_nhz.p);
        MPN_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(lr_mask_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const uint32_t *)d_cov.p, (const uint32_t *)d_badcol.p, m,
                       (uint32_t *)d_mask);
    MPN_HIP_CHECK(hipGetLastError());
    unsigned long long bad = LR_NONE;
    unsigned long long nhz = 0;
    if (tm.stop(st) || d_bad.download(&bad, 1, st) || d_nhz.download(&nhz, 1, st)) return -1;
    if (lr_time(tm, st, &tl_lr_ms[0])) return -1;
    lr_bad_out(bad, bad_pair, bad_why);
    *n_hazards = (int64_t)nhz;
    if ((int64_t)nhz > hazard_cap) {
        set_error("mpn_lr_columns: %lld hazards, room for %lld", (long long)nhz, (long long)hazard_cap);
        return -3;
    }
    if (nhz && bad == LR_NONE) {
        hipLaunchKernelGGL(lr_hazard_kernel, dim3((unsigned)nhz), dim3(64), 0, st, (const uint8_t *)d_text, text_len, (const mpn_lr_read *)d_reads.p,
                           (const mpn_lr_pair *)d_pairs.p, d_hz.p);
        MPN_HIP_CHECK(hipGetLastError());
    }
    if (nhz && d_hz.download(hazards, (size_t)nhz * 3, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int32_t mpn_lr_fragments(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_lr_read *reads, int64_t m, const int32_t *site_pos,
                                    int64_t n_pairs, const mpn_lr_pair *pairs, const void *d_mask, int32_t *len, int32_t *first, const int64_t *frag_off,
                                    void *d_letters, void *d_codes, int64_t cap, int64_t *bad_pair, int32_t *bad_why) {
    tl_lr_ms[1] = 0;
    const bool fill = d_letters != nullptr;
    if (!bad_pair || !bad_why || (n_pairs > 0 && (!d_mask || !len || (!fill && !first))) || (fill && (cap < 0 || (n_pairs > 0 && (!d_codes || !frag_off)))) ||
        !lr_common_args(d_text, text_len, n_reads, reads, m, site_pos, n_pairs, pairs)) {
        set_error("mpn_lr_fragments: bad arguments, a read that does not lie inside the text, a site at or before position 300, or a pair without its site or read");
        return -2;
    }
    if (fill)
        for (int64_t i = 0; i < n_pairs; ++i)
            if (frag_off[i] >= 0 && (len[i] < 0 || frag_off[i] + len[i] > cap)) {
                set_error("mpn_lr_fragments: the fragment of pair %lld does not fit the arena", (long long)i);
                return -3;
            }
    *bad_pair = -1; *bad_why = 0;
    if (n_pairs == 0) return 0;
    hipStream_t st = 0;
    DevBuf<mpn_lr_read> d_reads;
    DevBuf<mpn_lr_pair> d_pairs;
    DevBuf<int32_t> d_pos, d_len, d_first;
    DevBuf<int64_t> d_off;
    DevBuf<unsigned long long> d_bad;
    DevTimer tm;
    if (d_reads.upload(reads, (size_t)n_reads, st) || d_pairs.upload(pairs, (size_t)n_pairs, st) || d_pos.upload(site_pos, (size_t)m, st) ||
        (fill ? d_len.upload(len, (size_t)n_pairs, st) || d_off.upload(frag_off, (size_t)n_pairs, st) : d_len.alloc((size_t)n_pairs) || d_first.alloc((size_t)n_pairs)) ||
        d_bad.upload(&LR_NONE, 1, st) || tm.start(st))
        return -1;
    const dim3 grid((unsigned)((n_pairs + LR_WAVES - 1) / LR_WAVES));
    if (fill)
        hipLaunchKernelGGL(lr_frag_kernel<true>, grid, dim3(LR_THREADS), 0, st, (const uint8_t *)d_text, text_len, (const mpn_lr_read *)d_reads.p, n_reads,
                           (const int32_t *)d_pos.p, m, (const mpn_lr_pair *)d_pairs.p, n_pairs, (const uint32_t *)d_mask, d_len.p, (int32_t *)nullptr,
                           (const int64_t *)d_off.p, (uint8_t *)d_letters, (int8_t *)d_codes, cap, d_bad.p);
    else
        hipLaunchKernelGGL(lr_frag_kernel<false>, grid, dim3(LR_THREADS), 0, st, (const uint8_t *)d_text, text_len, (const mpn_lr_read *)d_reads.p, n_reads,
                           (const int32_t *)d_pos.p, m, (const mpn_lr_pair *)d_pairs.p, n_pairs, (const uint32_t *)d_mask, d_len.p, d_first.p,
                           (const int64_t *)nullptr, (uint8_t *)nullptr, (int8_t *)nullptr, (int64_t)0, d_bad.p);
    MPN_HIP_CHECK(hipGetLastError());
    unsigned long long bad = LR_NONE;
    if (tm.stop(st) || d_bad.download(&bad, 1, st) || (fill ? 0 : d_len.download(len, (size_t)n_pairs, st) || d_first.download(first, (size_t)n_pairs, st)))
        return -1;
    if (lr_time(tm, st, &tl_lr_ms[1])) return -1;
    lr_bad_out(bad, bad_pair, bad_why);
    return 0;
}

extern "C" int32_t mpn_lr_align_tally(int64_t m, const int32_t *site_pos, const int64_t *pair_begin, int64_t n_pairs, const int64_t *frag_off,
                                      const int32_t *frag_len, const void *d_letters, const void *d_codes, const void *d_contig, int64_t contig_len,
                                      int32_t *depth, int32_t *raises, int64_t *key_begin, void *d_keys, int64_t keys_cap, void *d_bytes, int64_t bytes_cap,
                                      int64_t *bad_pair, int32_t *bad_why) {
    tl_lr_ms[2] = tl_lr_ms[3] = 0;
    if (m < 0 || m > 0x7ffffff0 || n_pairs < 0 || n_pairs > 0x0ffffff0 || contig_len < 0 || contig_len > 0x7ffff000 || !bad_pair || !bad_why ||
        (m > 0 && (!site_pos || !pair_begin || !depth || !raises || !key_begin || !d_contig || !d_keys || !d_bytes)) ||
        (n_pairs > 0 && (!frag_off || !frag_len || !d_letters || !d_codes)) || keys_cap < 0 || bytes_cap < 0) {
        set_error("mpn_lr_align_tally: bad arguments");
        return -2;
    }
    *bad_pair = -1; *bad_why = 0;
    if (m == 0) return 0;
    if (pair_begin[0] != 0 || pair_begin[m] != n_pairs) {
        set_error("mpn_lr_align_tally: the sites do not partition the pairs");
        return -2;
    }
    std::vector<int32_t> pair_site((size_t)n_pairs), mask_len((size_t)n_pairs), ref_len((size_t)n_pairs);
    std::vector<int64_t> ref_off((size_t)n_pairs);
    for (int64_t c = 0; c < m; ++c) {
        if (pair_begin[c + 1] < pair_begin[c] || site_pos[c] <= MPN_LR_FLANK || site_pos[c] > contig_len) {
            set_error("mpn_lr_align_tally: site %lld: its pairs are not a range, or it does not lie behind position 300 and inside the contig", (long long)c);
            return -2;
        }
        const int64_t hi = std::min<int64_t>((int64_t)site_pos[c] + MPN_LR_FLANK, contig_len);
        for (int64_t i = pair_begin[c]; i < pair_begin[c + 1]; ++i) {
            if (frag_len[i] <= 0 || frag_off[i] < 0) {
                set_error("mpn_lr_align_tally: pair %lld has no fragment", (long long)i);
                return -2;
            }
            pair_site[i] = (int32_t)c;
            mask_len[i] = frag_len[i] <= 30 ? 15 : frag_len[i];       // pyssw.SSW.align
            ref_off[i] = c * MPN_LR_REF_STRIDE;
            ref_len[i] = (int32_t)(hi - ((int64_t)site_pos[c] - MPN_LR_FLANK - 1));
        }
    }
    // every pair gives at most MAX_KEYS keys; a key's text is at most 1 + the fragment, or 1 + the reference window
    hipStream_t st = 0;
    DevBuf<int32_t> d_pos, d_pair_site, d_frag_len;
    DevBuf<int64_t> d_pair_begin, d_frag_off;
    DevBuf<int8_t> d_refs;
    DevBuf<unsigned long long> d_bad;
    DevTimer tm;
    if (d_pos.upload(site_pos, (size_t)m, st) || d_pair_begin.upload(pair_begin, (size_t)m + 1, st) || d_pair_site.upload(pair_site.data(), (size_t)n_pairs, st) ||
        d_frag_off.upload(frag_off, (size_t)n_pairs, st) || d_frag_len.upload(frag_len, (size_t)n_pairs, st) || d_refs.alloc((size_t)m * MPN_LR_REF_STRIDE) ||
        d_bad.upload(&LR_NONE, 1, st) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(lr_refs_kernel, dim3((unsigned)((m * MPN_LR_REF_STRIDE + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_contig, contig_len,
                       (const int32_t *)d_pos.p, m, d_refs.p);
    MPN_HIP_CHECK(hipGetLastError());
    static const int8_t MAT[25] = {4, -6, -6, -6, 0, -6, 4, -6, -6, 0, -6, -6, 4, -6, 0, -6, -6, -6, 4, 0, 0, 0, 0, 0, 0};
    SswResident R;
    if (n_pairs > 0) {
        const int rc = ssw_resident((int32_t)n_pairs, (const int8_t *)d_codes, frag_off, frag_len, d_refs.p, ref_off.data(), ref_len.data(), MAT, 5, 2, 8, 2, 2,
                                    0, 0, mask_len.data(), R);
        if (rc) return rc;
    }
    if (tm.stop(st) || lr_time(tm, st, &tl_lr_ms[2])) return -1;

    DevBuf<LrKeyRef> d_keyref;
    DevBuf<int32_t> d_nkeys, d_refpos, d_rep, d_cnt, d_site_keys, d_depth, d_raises;
    DevBuf<unsigned long long> d_rank;
    DevBuf<int64_t> d_site_bytes, d_key_begin, d_byte_begin;
    const size_t slots = (size_t)n_pairs * MAX_KEYS;
    if (d_keyref.alloc(slots) || d_nkeys.alloc((size_t)n_pairs) || d_refpos.alloc((size_t)n_pairs) || d_rep.alloc(slots) || d_cnt.alloc(slots) ||
        d_rank.alloc(slots) || d_site_keys.alloc((size_t)m) || d_site_bytes.alloc((size_t)m) || d_depth.alloc((size_t)m) || d_raises.alloc((size_t)m) ||
        tm.start(st))
        return -1;
    if (n_pairs > 0) {
        hipLaunchKernelGGL(lr_keys_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, n_pairs, (const int32_t *)R.res.p,
                           (const uint32_t *)R.cig.p, (const int64_t *)R.cig_end.p, (const int32_t *)R.cig_len.p, (const int64_t *)d_frag_off.p,
                           (const int32_t *)d_frag_len.p, (const int32_t *)d_pair_site.p, (const int32_t *)d_pos.p, contig_len, d_keyref.p, d_nkeys.p,
                           d_refpos.p, d_bad.p);
        MPN_HIP_CHECK(hipGetLastError());
    }
    const LrTable tab{d_rep.p, d_cnt.p, d_rank.p};
    // (a site without pairs reads no result row)
    hipLaunchKernelGGL(lr_site_kernel, dim3((unsigned)m), dim3(64), 0, st, m, (const int64_t *)d_pair_begin.p, (const int32_t *)R.res.p,
                       (const LrKeyRef *)d_keyref.p, (const int32_t *)d_nkeys.p, (const int32_t *)d_refpos.p, (const uint8_t *)d_letters,
                       (const uint8_t *)d_contig, tab, d_site_keys.p, d_site_bytes.p, d_depth.p, d_raises.p);
    MPN_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> site_keys((size_t)m);
    std::vector<int64_t> site_bytes((size_t)m), byte_begin((size_t)m + 1, 0);
    unsigned long long bad = LR_NONE;
    if (d_site_keys.download(site_keys.data(), (size_t)m, st) || d_site_bytes.download(site_bytes.data(), (size_t)m, st) ||
        d_depth.download(depth, (size_t)m, st) || d_raises.download(raises, (size_t)m, st) || d_bad.download(&bad, 1, st))
        return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    lr_bad_out(bad, bad_pair, bad_why);
    key_begin[0] = 0;
    for (int64_t c = 0; c < m; ++c) {
        key_begin[c + 1] = key_begin[c] + site_keys[c];
        byte_begin[c + 1] = byte_begin[c] + site_bytes[c];
    }
    if (key_begin[m] > keys_cap || byte_begin[m] > bytes_cap) {
        set_error("mpn_lr_align_tally: %lld keys of %lld bytes do not fit the output (%lld, %lld)", (long long)key_begin[m], (long long)byte_begin[m],
                  (long long)keys_cap, (long long)bytes_cap);
        return -3;
    }
    if (bad == LR_NONE && key_begin[m] > 0) {
        if (d_key_begin.upload(key_begin, (size_t)m + 1, st) || d_byte_begin.upload(byte_begin.data(), (size_t)m + 1, st)) return -1;
        hipLaunchKernelGGL(lr_emit_kernel, dim3((unsigned)m), dim3(64), 0, st, m, (const int64_t *)d_pair_begin.p, (const LrKeyRef *)d_keyref.p,
                           (const uint8_t *)d_letters, (const uint8_t *)d_contig, tab, (const int32_t *)d_site_keys.p, (const int64_t *)d_key_begin.p,
                           (const int64_t *)d_byte_begin.p, (mpn_lr_key *)d_keys, keys_cap, (uint8_t *)d_bytes, bytes_cap);
        MPN_HIP_CHECK(hipGetLastError());
    }
    if (tm.stop(st)) return -1;
    return lr_time(tm, st, &tl_lr_ms[3]);
}

extern "C" int32_t mpn_ssw_align_resident(int32_t n_pairs, const void *d_reads, const int64_t *read_off, const int32_t *read_len, const void *d_refs,
                                          const int64_t *ref_off, const int32_t *ref_len, const int8_t *mat, int32_t n, int8_t score_size,
                                          uint8_t gap_open, uint8_t gap_extend, uint8_t flag, uint16_t filters, int32_t filterd, const int32_t *mask_len,
                                          void *d_res, void *d_cigar, int64_t cigar_cap, int64_t *cigar_off, int32_t *cigar_len, int32_t *status) {
    if (n_pairs < 0 || cigar_cap < 0 || (n_pairs > 0 && (!d_reads || !d_refs || !read_off || !read_len || !ref_off || !ref_len || !mat || !mask_len || !d_res ||
                                                        !cigar_off || !cigar_len || !status))) {
        set_error("mpn_ssw_align_resident: bad arguments");
        return -2;
    }
    if (n_pairs == 0) return 0;
    SswResident R;
    const int rc = ssw_resident(n_pairs, (const int8_t *)d_reads, read_off, read_len, (const int8_t *)d_refs, ref_off, ref_len, mat, n, score_size, gap_open,
                                gap_extend, flag, filters, filterd, mask_len, R);
    if (rc) return rc;
    if (R.cig_total > cigar_cap || (R.cig_total > 0 && !d_cigar)) {
        set_error("mpn_ssw_align_resident: the CIGARs need %lld entries, the caller has %lld", (long long)R.cig_total, (long long)cigar_cap);
        return -3;
    }
    hipStream_t st = 0;
    MPN_HIP_CHECK(hipMemcpyAsync(d_res, R.res.p, (size_t)n_pairs * 9 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (R.cig_total > 0) MPN_HIP_CHECK(hipMemcpyAsync(d_cigar, R.cig.p, (size_t)R.cig_total * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    for (int32_t i = 0; i < n_pairs; ++i) {
        status[i] = R.status_h[i];
        const bool has = R.status_h[i] == MPN_SSW_OK && R.cig_len_h[i] > 0;
        cigar_len[i] = has ? R.cig_len_h[i] : 0;
        cigar_off[i] = has ? R.cig_end_h[i] - R.cig_len_h[i] : 0;
    }
    return 0;
}
