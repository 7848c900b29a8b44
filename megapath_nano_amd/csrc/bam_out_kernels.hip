// The device BAM writer behind include/mpn_bam.h (mpn_bam_out_*, mpn_sam_encode_batch, mpn_bai_build): the work of
// `samtools view -F.. -b | samtools sort; samtools index` with the records resident between the SAM text and the deflate.  Every
// rule that decides a byte is in bam_out_core.h, which the host check runs serially; the kernels here spread the same work over a wave.
//
//   bo_lf_count / bo_lf_fill / bo_line_len   line starts of a chunk of text from its line feeds (a block takes 4 KiB, a lane 16 bytes)
//   bo_scan_kernel      a wave per line, 64 bytes a step: ballots over tabs, carriage returns and white space give the eleven tab
//                       positions; seven lanes take FLAG POS MAPQ PNEXT TLEN and the two reference names (name_set_core.h); the
//                       CIGAR walk counts operations and reference bases; the aux walk sizes every field -> BoRec
//   bo_offsets_kernel   exclusive scan of the record sizes
//   bo_encode_kernel    a wave per line: fixed part, QNAME, CIGAR words (or the 2-operation stand-in + CG:B,I), packed SEQ, QUAL,
//                       aux fields; every output byte is written once
//   bo_gather_kernel    sorted records + their block_size words + the BAM header -> the payload stream of a round of blocks, in
//                       output-owned 16-byte chunks (gather16.h), pieces found by binary search in their ascending starts
// CIGAR walk: a ballot of the non-digit bytes of a step; a lane that holds an operation letter knows the letter before it (the
// highest set bit below its own, or the last one of an earlier step), so its number is the digits between them, wherever a step
// boundary falls, and the prefix count of the ballot is its index.  Aux walk: steps are taken from the END of the line, so that the
// tab that ends a field is known (the lowest set bit above, or the first tab of a later step); sizes are summed as suffix sums,
// which place every field from the end of the aux block.  A lane encodes its own field; the text of a long Z / H value is copied
// by the whole wave.
// The coordinate sort is mpn_sort_order; the block cut (BoCut) and the index (bai_build) are serial chains and run on the host
// from the 64-byte summaries the scan leaves.
#include "bam_out_core.h"
#include "bgzf_resident.h"
#include "name_set_dev.h"
#include "../../include/mpn_abundance.h"
#include "../../include/mpn_ingest.h"

#include <chrono>
#include <cstring>
#include <string>

namespace mpn {

using namespace bo;

constexpr int BO_LF_BLOCK = 4096;           // bytes of text a block of the line-start kernels takes
constexpr int BO_LONG_VALUE = 32;           // a Z / H text of more bytes is copied by the wave, not by its lane
constexpr int BO_MAX_GRID = 256 * 32;       // waves in flight for the per-line kernels; more lines are taken in rounds

struct BoNames {                            // the resident name set, as a kernel argument
    const NsSlot *table;
    const uint4 *pool;
    uint32_t mask;
};

__device__ __forceinline__ uint64_t lanes_below(int lane) { return ((uint64_t)1 << lane) - 1; }
__device__ __forceinline__ uint64_t lanes_above(int lane) { return lane == 63 ? 0 : ~(((uint64_t)2 << lane) - 1); }
__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// the smallest status above 0 among the lanes, 0 if there is none
__device__ __forceinline__ int32_t wave_worst(int32_t st) {
    const int32_t m = wave_reduce_min(st == 0 ? 0x7fffffff : st);
    return m == 0x7fffffff ? 0 : m;
}

// ---- line starts -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int bo_lf_mask16(const uint8_t *__restrict__ text, int64_t len, int64_t at) {
    int m = 0;
    if (at + 16 <= len) {
        const uint4 v = *(const uint4 *)(text + at);      // (text is 16-byte aligned and `at` a multiple of 16)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) m |= (((w[k >> 2] >> (8 * (k & 3))) & 0xff) == '\n') << k;
    } else {
        for (int k = 0; k < 16 && at + k < len; ++k) m |= (text[at + k] == '\n') << k;
    }
    return m;
}

__global__ __launch_bounds__(256) void bo_lf_count_kernel(const uint8_t *__restrict__ text, int64_t len, int32_t *__restrict__ counts) {
    __shared__ int part[4];
    const int64_t at = (int64_t)blockIdx.x * BO_LF_BLOCK + 16 * threadIdx.x;
    const int c = wave_scan_add(__popc(bo_lf_mask16(text, len, at)));
    if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// first[i]: line feeds before block i.  Line g + 1 starts behind line feed g; line 0 starts at 0 (the host sets it).
__global__ __launch_bounds__(256) void bo_lf_fill_kernel(const uint8_t *__restrict__ text, int64_t len, const int64_t *__restrict__ first,
                                                         int64_t *__restrict__ line_start) {
    __shared__ int part[4];
    const int64_t at = (int64_t)blockIdx.x * BO_LF_BLOCK + 16 * threadIdx.x;
    int m = bo_lf_mask16(text, len, at);
    const int own = __popc(m), incl = wave_scan_add(own), wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) part[wave] = incl;
    __syncthreads();
    int64_t g = first[blockIdx.x] + incl - own;
    for (int w = 0; w < wave; ++w) g += part[w];
    while (m) {
        const int k = __ffs(m) - 1;
        m &= m - 1;
        line_start[++g] = at + k + 1;
    }
}

// one block: out[i] = the counts before i, out[n] = all of them
__global__ __launch_bounds__(1024) void bo_offsets_kernel(const int32_t *__restrict__ v, int64_t stride, int64_t n, int64_t *__restrict__ out) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int64_t sum = 0;
    for (int64_t k = lo; k < hi; ++k) sum += v[k * stride];
    part[t] = sum;
    __syncthreads();
    if (t == 0) { int64_t acc = 0; for (int k = 0; k < 1024; ++k) { const int64_t x = part[k]; part[k] = acc; acc += x; } out[n] = acc; }
    __syncthreads();
    int64_t o = part[t];
    for (int64_t k = lo; k < hi; ++k) { out[k] = o; o += v[k * stride]; }
}

// line i is text[line_start[i] .. line_start[i + 1]) with its line feed: the length without it
__global__ __launch_bounds__(256) void bo_line_len_kernel(const int64_t *__restrict__ line_start, int64_t n, int32_t *__restrict__ line_len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) line_len[i] = (int32_t)(line_start[i + 1] - line_start[i] - 1);
}

// ---- the two walks -----------------------------------------------------------------------------------------------------------------
// f(k, op, num) in the lane that holds operation k of the CIGAR p[a .. b); *st takes the lane's faults.  -> the operations
template <class F>
__device__ __forceinline__ int32_t bo_wave_cigar(const uint8_t *__restrict__ p, int32_t a, int32_t b, int lane, int32_t *st, F f) {
    if (b - a == 1 && p[a] == '*') return 0;
    int32_t n_ops = 0, last = a - 1;          // last: the last byte before this step that is no digit (the same in all lanes)
    for (int32_t s = a; s < b; s += 64) {
        const int32_t i = s + lane;
        const bool letter = i < b && !bo_is_digit(p[i]);
        const uint64_t m = __ballot(letter);
        if (letter) {
            const uint64_t below = m & lanes_below(lane);
            const int32_t prev = below ? s + 63 - __clzll((long long)below) : last;
            int op;
            int64_t num;
            const int32_t s1 = bo_cigar_one(p, prev + 1, i, &op, &num);
            if (s1) *st = bo_worse(*st, s1);
            else f(n_ops + __popcll(below), op, num);
        }
        if (m) last = s + 63 - __clzll((long long)m);
        n_ops += __popcll(m);
    }
    if (last != b - 1 && lane == 0) *st = bo_worse(*st, MPN_SAM_CIGAR_NUM);      // digits without an operation behind them
    return n_ops;
}

// Every lane calls f(has, a, b, behind) once per step: has -- the lane holds the tab in front of the aux field p[a .. b); behind --
// the sizes f returned for the fields of later steps.  f returns the field's size (0 without one).  -> the sizes of all fields
template <class F>
__device__ __forceinline__ int64_t bo_wave_aux(const uint8_t *__restrict__ p, int32_t from, int32_t len, int lane, F f) {
    int64_t behind = 0;
    int32_t next = len;                        // the first tab of the steps behind this one, or the end of the line
    for (int32_t s = from + ((len - from - 1) & ~63); s >= from && from < len; s -= 64) {
        const int32_t i = s + lane;
        const bool tab = i < len && p[i] == '\t';
        const uint64_t m = __ballot(tab), above = m & lanes_above(lane);
        const int32_t end = above ? s + __ffsll((long long)above) - 1 : next;
        behind += f(tab, i + 1, end, behind);
        if (m) next = s + __ffsll((long long)m) - 1;
    }
    return behind;
}

// ---- scan ----------------------------------------------------------------------------------------------------------------------------
// A block is one wave, so that __syncthreads orders the wave's LDS traffic.  text_al: 16-byte aligned; a line lies at text_al + off.
__global__ __launch_bounds__(64) void bo_scan_kernel(const uint8_t *__restrict__ text_al, const int64_t *__restrict__ line_off, const int32_t *__restrict__ line_len,
                                                     int64_t n, BoNames names, int32_t exclude_flags, int32_t *__restrict__ tabs, BoRec *__restrict__ recs) {
    __shared__ int32_t tab[11];
    __shared__ BoRec rec;
    const int lane = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const int64_t off = line_off[r];
        const uint8_t *__restrict__ p = text_al + off;
        int32_t len = line_len[r];
        if (len > 0 && p[len - 1] == '\n') --len;
        __syncthreads();                          // the previous line's tab[] and rec have been read
        if (lane < 16) ((int32_t *)&rec)[lane] = 0;
        int32_t n_tab = 0;
        bool cr = false, text = false;
        for (int32_t s = 0; s < len; s += 64) {
            const int32_t i = s + lane;
            const uint8_t c = i < len ? p[i] : (uint8_t)' ';
            const uint64_t m = __ballot(c == '\t');
            const int32_t k = n_tab + __popcll(m & lanes_below(lane));
            if (c == '\t' && k < 11) tab[k] = i;
            cr |= __ballot(c == '\r') != 0;
            text |= __ballot(!bo_is_space(c)) != 0;
            n_tab += __popcll(m);
        }
        int32_t status = 0;
        if ((len > 0 && p[0] == '@') || !text) status = MPN_SAM_SKIPPED;
        else if (cr) status = MPN_SAM_CR;
        else if (n_tab < 10) status = MPN_SAM_FEW_FIELDS;
        if (n_tab == 10 && lane == 0) tab[10] = len;
        __syncthreads();
        if (status == 0) {
            // FLAG first: an excluded line is never looked at again
            int32_t st = 0;
            if (lane == 0) st = bo_numeric_field(p, tab, 0, &rec);
            st = __shfl(st, 0);
            __syncthreads();
            if (st) status = st;
            else if (rec.flag & exclude_flags) status = MPN_SAM_EXCLUDED;
        }
        if (status == 0) {
            int32_t st = 0;
            if (lane >= 1 && lane < 5) st = bo_numeric_field(p, tab, lane, &rec);
            if (lane == 5 || lane == 6) {
                const int k = lane == 5 ? 2 : 6;
                const int32_t a = bo_field_start(tab, k), nb = tab[k] - a;
                int32_t id;
                if (nb == 1 && (p[a] == '*' || (k == 6 && p[a] == '='))) id = p[a] == '*' ? -1 : -2;      // -2: RNEXT is RNAME
                else {
                    const NsTextWords w{(const uint4 *)text_al, off + a, nb};
                    id = ns_find(names.table, names.mask, ns_hash(nb, w), nb, w, NsDevPool{names.pool});
                }
                if (k == 2) rec.tid = id; else rec.ntid = id;
            }
            int64_t ref = 0;
            const int32_t n_ops = bo_wave_cigar(p, bo_field_start(tab, 5), tab[5], lane, &st, [&](int32_t, int op, int64_t num) { if (bo_ref_consuming(op)) ref += num; });
            ref = wave_sum64(ref);
            const int64_t aux = bo_wave_aux(p, tab[10], len, lane, [&](bool has, int32_t a, int32_t b, int64_t) -> int64_t {
                BoAux x;
                x.size = 0;
                if (has) st = bo_worse(st, bo_aux_head(p, a, b, &x));
                return wave_sum64(x.size);
            });
            if (lane == 0) {
                const int32_t a = bo_field_start(tab, 9), nb = tab[9] - a;
                const int32_t l_seq = (nb == 1 && p[a] == '*') ? 0 : nb;
                const int32_t qa = bo_field_start(tab, 10), qn = tab[10] - qa;
                if (l_seq > 0 && !(qn == 1 && p[qa] == '*') && qn != l_seq) st = bo_worse(st, MPN_SAM_QUAL_LEN);
                if (aux > 0x7fffffffLL) st = bo_worse(st, MPN_SAM_NUM_RANGE);
                rec.l_seq = l_seq;
                rec.n_ops = n_ops;
                rec.aux_size = aux > 0x7fffffffLL ? 0 : (int32_t)aux;
            }
            __syncthreads();                      // every lane's fields are in rec
            if (lane == 0) {
                if (rec.ntid == -2) rec.ntid = rec.tid;
                st = bo_worse(st, bo_finish_rec(tab, ref, &rec));
            }
            status = wave_worst(st);
        }
        __syncthreads();
        if (lane == 0) { rec.status = status; if (status) rec.size = 0; if (status == MPN_SAM_SKIPPED) rec.flag = text; }      // flag 1: a header line
        __syncthreads();
        if (lane < 16) ((int32_t *)&recs[r])[lane] = ((const int32_t *)&rec)[lane];
        if (lane < 11) tabs[11 * r + lane] = tab[lane];
    }
}

// ---- encode ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void bo_encode_kernel(const uint8_t *__restrict__ text_al, const int64_t *__restrict__ line_off, const int32_t *__restrict__ line_len,
                                                       int64_t n, const int32_t *__restrict__ tabs, const BoRec *__restrict__ recs,
                                                       const int64_t *__restrict__ rec_off, uint8_t *__restrict__ pool) {
    const int lane = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const BoRec rec = recs[r];
        if (rec.status != MPN_SAM_OK) continue;
        const uint8_t *__restrict__ p = text_al + line_off[r];
        int32_t len = line_len[r];
        if (len > 0 && p[len - 1] == '\n') --len;
        int32_t tab[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) tab[k] = tabs[11 * r + k];
        uint8_t *__restrict__ out = pool + rec_off[r];
        const int32_t l_name = tab[0] + 1;
        const bool long_cigar = rec.n_ops > BO_MAX_CIGAR_OPS;
        uint8_t *o = out + 32;
        if (lane == 0) { bo_put_fixed(rec, l_name, out); o[tab[0]] = 0; }
        for (int32_t i = lane; i < tab[0]; i += 64) o[i] = p[i];
        o += l_name;
        uint8_t *cg = out + rec.size - 4 * (int64_t)rec.n_ops;     // where the real CIGAR goes when it is long
        if (long_cigar && lane == 0) {
            bo_put32(o, (uint32_t)rec.l_seq << 4 | 4u);
            bo_put32(o + 4, (uint32_t)rec.ref_len << 4 | 3u);
            cg[-8] = 'C'; cg[-7] = 'G'; cg[-6] = 'B'; cg[-5] = 'I';
            bo_put32(cg - 4, (uint32_t)rec.n_ops);
        }
        {
            uint8_t *words = long_cigar ? cg : o;
            int32_t st = 0;
            bo_wave_cigar(p, tab[4] + 1, tab[5], lane, &st, [&](int32_t k, int op, int64_t num) { bo_put32(words + 4 * (int64_t)k, (uint32_t)num << 4 | (uint32_t)op); });
        }
        o += long_cigar ? 8 : 4 * (int64_t)rec.n_ops;
        const uint8_t *__restrict__ sq = p + tab[8] + 1;
        const int32_t n_packed = (rec.l_seq + 1) / 2;
        for (int32_t j = lane; j < n_packed; j += 64)
            o[j] = (uint8_t)(bo_seq_code(sq[2 * j]) << 4 | (2 * j + 1 < rec.l_seq ? bo_seq_code(sq[2 * j + 1]) : 0));
        o += n_packed;
        const int32_t qa = tab[9] + 1;
        const bool no_qual = tab[10] - qa == 1 && p[qa] == '*';
        for (int32_t j = lane; j < rec.l_seq; j += 64) o[j] = no_qual ? (uint8_t)0xff : (uint8_t)(p[qa + j] - 33);
        o += rec.l_seq;
        uint8_t *aux_end = o + rec.aux_size;
        bo_wave_aux(p, tab[10], len, lane, [&](bool has, int32_t a, int32_t b, int64_t behind) -> int64_t {
            BoAux x;
            x.size = 0; x.width = 1;
            if (has) bo_aux_head(p, a, b, &x);
            // suffix sums: the fields of the lanes above, in this step, lie behind this lane's
            const int32_t incl = wave_scan_add(x.size), total = __shfl(incl, 63);
            uint8_t *dst = aux_end - behind - (total - incl + x.size);
            const bool text_value = has && x.width == 0;
            const int32_t n_text = text_value ? x.size - 4 : 0;
            if (has) bo_aux_put(p, a, x, dst);
            if (text_value && n_text <= BO_LONG_VALUE)
                for (int32_t k = 0; k < n_text; ++k) dst[3 + k] = p[a + 5 + k];
            uint64_t big = __ballot(n_text > BO_LONG_VALUE);
            while (big) {                          // (the same in all lanes)
                const int l = __ffsll((long long)big) - 1;
                big &= big - 1;
                const int32_t src = __shfl(a, l) + 5, cnt = __shfl(n_text, l);
                const uint64_t d64 = __shfl((unsigned long long)(uintptr_t)dst, l);
                uint8_t *d = (uint8_t *)(uintptr_t)d64 + 3;
                for (int32_t k = lane; k < cnt; k += 64) d[k] = p[src + k];
            }
            return total;
        });
    }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------------------
// The payload stream: header[0 .. header_len), then per sorted record k its block_size word and its bytes; piece k starts at
// start[k] (ascending, start[n] = the end of the stream) and its record lies at pool + src[k].  A lane owns 16 aligned bytes of
// out, which receives stream[s0 .. s1): each is one 16-byte store.
__global__ __launch_bounds__(G16_THREADS) void bo_gather_kernel(const uint8_t *__restrict__ header, int64_t header_len, const int64_t *__restrict__ start,
                                                                const int64_t *__restrict__ src, int64_t n, const uint8_t *__restrict__ pool,
                                                                int64_t s0, int64_t s1, uint4 *__restrict__ out) {
    const int64_t n16 = (s1 - s0 + 15) / 16;
    for (int64_t v = (int64_t)blockIdx.x * G16_THREADS + threadIdx.x; v < n16; v += (int64_t)gridDim.x * G16_THREADS) {
        const int64_t q = s0 + 16 * v;             // the stream offset of the lane's first byte
        int64_t k = q < header_len ? -1 : last_le(start, 0, n - 1, q);
        uint4 res;
        if (k >= 0 && q >= start[k] + 4 && q + 16 <= start[k + 1] && q + 16 <= s1) res = load16(pool + src[k] + (q - start[k] - 4));
        else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int b = 0; b < 16 && q + b < s1; ++b) {
                const int64_t at = q + b;
                while (k + 1 < n && at >= start[k + 1]) ++k;      // (from the header into piece 0, or into the next piece)
                uint32_t c;
                if (at < header_len) c = header[at];
                else {
                    const int64_t in = at - start[k];
                    c = in < 4 ? ((uint32_t)(start[k + 1] - start[k] - 4) >> (8 * in)) & 0xff : pool[src[k] + in - 4];
                }
                w[b >> 2] |= c << (8 * (b & 3));
            }
            res = make_uint4(w[0], w[1], w[2], w[3]);
        }
        out[v] = res;
    }
}

const char *const BO_STATUS_TEXT[MPN_SAM_N_STATUS] = {
    "ok", "no record (header or blank line)", "excluded by its flags", "fewer than 11 fields",
    "FLAG, POS, MAPQ, PNEXT or TLEN is not a number", "a numeric field is out of range", "QNAME longer than 254 bytes",
    "unknown CIGAR operation", "CIGAR operation without a number or above 2^28-1", "SEQ and QUAL of different lengths",
    "malformed optional field", "integer tag malformed or out of range", "float tag outside the forms the device takes",
    "array tag", "unknown tag type", "carriage return in the line", "the record pool would pass its limit",
    "header line behind a record"};

// ---- host: the per-line launches ---------------------------------------------------------------------------------------------------
struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

struct BoLines {                       // the resident lines of one chunk and what the scan left
    DevBuf<int64_t> line_off, rec_off;
    DevBuf<int32_t> line_len, tabs;
    DevBuf<BoRec> recs;
};

inline int bo_line_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(n, BO_MAX_GRID)); }

// scan + sizes -> L.recs, L.tabs, L.rec_off; h_recs and *total on the host when the call returns
static int bo_scan_lines(const uint8_t *d_text, BoLines &L, int64_t n, const mpn_name_set *set, int32_t exclude_flags, std::vector<BoRec> &h_recs,
                         int64_t *total, hipStream_t st, double *scan_ms) {
    DevTimer tm;
    h_recs.resize((size_t)n);
    int64_t h_total = 0;
    if (L.tabs.alloc((size_t)n * 11) || L.recs.alloc((size_t)n) || L.rec_off.alloc((size_t)n + 1) || tm.start(st)) return -1;
    const BoNames names{set->d_table, set->d_pool, (uint32_t)(set->slots - 1)};
    hipLaunchKernelGGL(bo_scan_kernel, dim3(bo_line_grid(n)), dim3(64), 0, st, d_text, (const int64_t *)L.line_off.p, (const int32_t *)L.line_len.p, n, names,
                       exclude_flags, L.tabs.p, L.recs.p);
    hipLaunchKernelGGL(bo_offsets_kernel, dim3(1), dim3(1024), 0, st, (const int32_t *)&L.recs.p->size, (int64_t)(sizeof(BoRec) / 4), n, L.rec_off.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st) || L.recs.download(h_recs.data(), (size_t)n, st)) return -1;
    MPN_HIP_CHECK(hipMemcpyAsync(&h_total, L.rec_off.p + n, 8, hipMemcpyDeviceToHost, st));
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    double ms = 0;
    if (tm.elapsed_ms(&ms)) return -1;
    if (scan_ms) *scan_ms += ms;
    *total = h_total;
    return 0;
}

// the records of the scanned lines -> d_out[0 .. total)
static int bo_encode_lines(const uint8_t *d_text, const BoLines &L, int64_t n, uint8_t *d_out, hipStream_t st, double *encode_ms) {
    DevTimer tm;
    if (tm.start(st)) return -1;
    hipLaunchKernelGGL(bo_encode_kernel, dim3(bo_line_grid(n)), dim3(64), 0, st, d_text, (const int64_t *)L.line_off.p, (const int32_t *)L.line_len.p, n,
                       (const int32_t *)L.tabs.p, (const BoRec *)L.recs.p, (const int64_t *)L.rec_off.p, d_out);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    double ms = 0;
    if (tm.elapsed_ms(&ms)) return -1;
    if (encode_ms) *encode_ms += ms;
    return 0;
}

static mpn_name_set *bo_name_set(const char *const *ref_names, int32_t n_ref) {
    std::string pool;
    std::vector<int64_t> off((size_t)n_ref + 1, 0);
    for (int32_t i = 0; i < n_ref; ++i) {
        pool += ref_names[i] ? ref_names[i] : "";
        off[(size_t)i + 1] = (int64_t)pool.size();
    }
    mpn_name_set *set = nullptr;
    if (mpn_name_set_create(n_ref, pool.data(), off.data(), 0, &set, nullptr)) return nullptr;
    return set;
}

}  // namespace mpn

using namespace mpn;

enum { ST_UPLOAD, ST_SCAN, ST_ENCODE, ST_SORT, ST_GATHER, ST_DEFLATE, ST_DOWNLOAD, ST_FILE, ST_CUT_BAI, ST_N };

struct mpn_bam_out {
    mpn_name_set *names = nullptr;
    int32_t n_ref = 0, exclude_flags = 0;
    int64_t chunk_bytes = 0, pool_bytes = 0;
    std::vector<char> pending;              // text that has not gone to the device yet: it ends inside a line, or is less than a chunk
    int64_t lines_before = 0;               // lines of the chunks that have gone
    int64_t refused_line = 0;
    int32_t refused_status = 0;
    bool finished = false, seen_record = false;
    DevBuf<uint8_t> pool;                   // the records, one behind the other in the order of the text
    int64_t pool_used = 0;
    std::vector<int32_t> tid, pos0, end0, flag, size;     // per record, in the order of the text
    std::vector<int64_t> src;               // where it lies in the pool
    double ms[ST_N] = {0};
};

extern "C" const char *mpn_sam_status_text(int32_t status) { return status >= 0 && status < MPN_SAM_N_STATUS ? BO_STATUS_TEXT[status] : "unknown status"; }

extern "C" int64_t mpn_bai_build(int32_t n_ref, int64_t n, const int32_t *tid, const int32_t *pos0, const int32_t *end0, const uint64_t *voff_after,
                                 const uint8_t *mapped, uint64_t voff_first, uint64_t voff_end, uint8_t *out, int64_t out_cap, int64_t *need) {
    if (n_ref < 0 || n < 0 || out_cap < 0 || (out_cap > 0 && !out) || (n > 0 && (!tid || !pos0 || !end0 || !voff_after || !mapped))) {
        set_error("mpn_bai_build: bad arguments");
        return -2;
    }
    const std::vector<uint8_t> bai = bai_build(n_ref, n, tid, pos0, end0, voff_after, mapped, voff_first, voff_end);
    if (need) *need = (int64_t)bai.size();
    if ((int64_t)bai.size() > out_cap) return -3;
    memcpy(out, bai.data(), bai.size());
    return (int64_t)bai.size();
}

extern "C" int64_t mpn_sam_encode_batch(const char *const *ref_names, int32_t n_ref, const char *text, const int64_t *line_off, const int32_t *line_len,
                                        int64_t n, int32_t exclude_flags, uint8_t *out, int64_t out_cap, int64_t *rec_off, int32_t *tid, int32_t *pos0,
                                        int32_t *end0, int32_t *flag, int32_t *status) {
    if (n_ref < 0 || (n_ref > 0 && !ref_names) || n < 0 || out_cap < 0 || (out_cap > 0 && !out) || !rec_off ||
        (n > 0 && (!text || !line_off || !line_len || !tid || !pos0 || !end0 || !flag || !status))) {
        set_error("mpn_sam_encode_batch: bad arguments");
        return -2;
    }
    rec_off[0] = 0;
    if (n == 0) return 0;
    int64_t text_len = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (line_off[i] < 0 || line_len[i] < 0) { set_error("mpn_sam_encode_batch: line %lld has a negative offset or length", (long long)i); return -2; }
        text_len = std::max(text_len, line_off[i] + line_len[i]);
    }
    mpn_name_set *set = bo_name_set(ref_names, n_ref);
    if (!set) return -1;
    struct Free { mpn_name_set *s; ~Free() { mpn_name_set_free(s); } } free_set{set};
    hipStream_t st = 0;
    DevBuf<uint8_t> d_text, d_out;
    BoLines L;
    std::vector<BoRec> recs;
    int64_t total = 0;
    if (d_text.alloc((size_t)text_len + 32)) return -1;           // (the name reader loads whole 16-byte vectors)
    MPN_HIP_CHECK(hipMemcpyAsync(d_text.p, text, (size_t)text_len, hipMemcpyHostToDevice, st));
    if (L.line_off.upload(line_off, (size_t)n, st) || L.line_len.upload(line_len, (size_t)n, st)) return -1;
    if (bo_scan_lines(d_text.p, L, n, set, exclude_flags, recs, &total, st, nullptr)) return -1;
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        const BoRec &r = recs[(size_t)i];
        rec_off[i] = at;
        at += r.size;
        tid[i] = r.tid; pos0[i] = r.pos0; end0[i] = r.end0; flag[i] = r.flag; status[i] = r.status;
    }
    rec_off[n] = at;
    if (at != total) { set_error("mpn_sam_encode_batch: the size scan disagrees with the sizes"); return -1; }
    if (total > out_cap) return -3;
    if (d_out.alloc((size_t)total + 16) || bo_encode_lines(d_text.p, L, n, d_out.p, st, nullptr)) return -1;
    if (d_out.download(out, (size_t)total, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return total;
}

extern "C" mpn_bam_out *mpn_bam_out_create(const char *const *ref_names, int32_t n_ref, int32_t exclude_flags, int64_t chunk_bytes, int64_t pool_bytes) {
    if (n_ref < 0 || (n_ref > 0 && !ref_names) || chunk_bytes < 1 || chunk_bytes > 0x7fffffffLL || pool_bytes < 0) {
        set_error("mpn_bam_out_create: bad arguments");
        return nullptr;
    }
    mpn_bam_out *w = new mpn_bam_out;
    w->names = bo_name_set(ref_names, n_ref);
    if (!w->names) { delete w; return nullptr; }
    w->n_ref = n_ref;
    w->exclude_flags = exclude_flags;
    w->chunk_bytes = chunk_bytes;
    w->pool_bytes = pool_bytes;
    return w;
}

extern "C" void mpn_bam_out_destroy(mpn_bam_out *w) {
    if (!w) return;
    mpn_name_set_free(w->names);
    delete w;
}

extern "C" int32_t mpn_bam_out_refusal(const mpn_bam_out *w, int64_t *line_no, int32_t *status) {
    if (!w || !w->refused_status) return 0;
    if (line_no) *line_no = w->refused_line;
    if (status) *status = w->refused_status;
    return 1;
}

extern "C" void mpn_bam_out_stage_ms(const mpn_bam_out *w, double *ms9) {
    for (int k = 0; k < ST_N; ++k) ms9[k] = w ? w->ms[k] : 0;
}

// one chunk of whole lines (its last byte is a line feed) through line starts, scan and encode.  0, 1 (refused) or -1
static int bo_take_chunk(mpn_bam_out *w, const char *text, int64_t len) {
    if (len > 0x7fffffffLL) { set_error("mpn_bam_out: a line of more than 2^31 - 1 bytes"); return -1; }
    hipStream_t st = 0;
    DevBuf<uint8_t> d_text;
    DevBuf<int32_t> counts;
    DevBuf<int64_t> first;
    BoLines L;
    const Clock up;
    if (d_text.alloc((size_t)len + 32)) return -1;
    MPN_HIP_CHECK(hipMemcpyAsync(d_text.p, text, (size_t)len, hipMemcpyHostToDevice, st));
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    w->ms[ST_UPLOAD] += up.ms();
    const int64_t n_blk = (len + BO_LF_BLOCK - 1) / BO_LF_BLOCK;
    int64_t n = 0;
    DevTimer tm;
    if (counts.alloc((size_t)n_blk) || first.alloc((size_t)n_blk + 1) || tm.start(st)) return -1;
    hipLaunchKernelGGL(bo_lf_count_kernel, dim3((unsigned)n_blk), dim3(256), 0, st, (const uint8_t *)d_text.p, len, counts.p);
    hipLaunchKernelGGL(bo_offsets_kernel, dim3(1), dim3(1024), 0, st, (const int32_t *)counts.p, (int64_t)1, n_blk, first.p);
    MPN_HIP_CHECK(hipGetLastError());
    MPN_HIP_CHECK(hipMemcpyAsync(&n, first.p + n_blk, 8, hipMemcpyDeviceToHost, st));
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (n < 1) { set_error("mpn_bam_out: a chunk without a line feed"); return -1; }
    if (L.line_off.alloc((size_t)n + 1) || L.line_len.alloc((size_t)n)) return -1;
    MPN_HIP_CHECK(hipMemsetAsync(L.line_off.p, 0, 8, st));
    hipLaunchKernelGGL(bo_lf_fill_kernel, dim3((unsigned)n_blk), dim3(256), 0, st, (const uint8_t *)d_text.p, len, (const int64_t *)first.p, L.line_off.p);
    hipLaunchKernelGGL(bo_line_len_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int64_t *)L.line_off.p, n, L.line_len.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    double lf_ms = 0;
    if (tm.elapsed_ms(&lf_ms)) return -1;
    w->ms[ST_SCAN] += lf_ms;
    std::vector<BoRec> recs;
    int64_t total = 0;
    if (bo_scan_lines(d_text.p, L, n, w->names, w->exclude_flags, recs, &total, st, &w->ms[ST_SCAN])) return -1;
    for (int64_t i = 0; i < n; ++i) {
        const BoRec &r = recs[(size_t)i];
        const bool late = r.status == MPN_SAM_SKIPPED && r.flag && w->seen_record;     // the header went into the file's before the text came
        if (bo_refused(r.status) || late) {
            w->refused_line = w->lines_before + i + 1;
            w->refused_status = late ? (int32_t)MPN_SAM_LATE_HEADER : r.status;
            return 1;
        }
        w->seen_record |= r.status != MPN_SAM_SKIPPED;
    }
    if (w->pool_used + total > w->pool_bytes) {
        // the first line whose record no longer fits
        int64_t at = w->pool_used, i = 0;
        while (i < n && at + recs[(size_t)i].size <= w->pool_bytes) at += recs[(size_t)i++].size;
        w->refused_line = w->lines_before + std::min(i, n - 1) + 1;
        w->refused_status = MPN_SAM_POOL;
        return 1;
    }
    if ((int64_t)w->pool.n < w->pool_used + total + 16) {          // grow: the records so far move once per doubling
        DevBuf<uint8_t> grown;
        const int64_t want = std::max<int64_t>(w->pool_used + total + 16, std::min<int64_t>(2 * (int64_t)w->pool.n, w->pool_bytes + 16));
        if (grown.alloc((size_t)want)) return -1;
        if (w->pool_used) MPN_HIP_CHECK(hipMemcpyAsync(grown.p, w->pool.p, (size_t)w->pool_used, hipMemcpyDeviceToDevice, st));
        MPN_HIP_CHECK(hipStreamSynchronize(st));
        std::swap(w->pool.p, grown.p);
        std::swap(w->pool.n, grown.n);
        std::swap(w->pool.owned, grown.owned);
    }
    if (total > 0 && bo_encode_lines(d_text.p, L, n, w->pool.p + w->pool_used, st, &w->ms[ST_ENCODE])) return -1;
    int64_t at = w->pool_used;
    for (int64_t i = 0; i < n; ++i) {
        const BoRec &r = recs[(size_t)i];
        if (r.status != MPN_SAM_OK) continue;
        w->tid.push_back(r.tid); w->pos0.push_back(r.pos0); w->end0.push_back(r.end0); w->flag.push_back(r.flag); w->size.push_back(r.size);
        w->src.push_back(at);
        at += r.size;
    }
    w->pool_used += total;
    w->lines_before += n;
    return 0;
}

// whole chunks out of pending; all of it if `last`
static int bo_drain(mpn_bam_out *w, bool last) {
    std::vector<char> &t = w->pending;
    if (last && !t.empty() && t.back() != '\n') t.push_back('\n');
    int64_t from = 0;
    const int64_t size = (int64_t)t.size();
    int rc = 0;
    while (from < size) {
        int64_t end = -1;                         // one behind the line feed that ends the chunk
        if (size - from <= w->chunk_bytes) { if (last) end = size; }
        else {
            for (int64_t q = from + w->chunk_bytes - 1; q >= from; --q) if (t[(size_t)q] == '\n') { end = q + 1; break; }
            if (end < 0) {                        // a line longer than a chunk is taken whole
                const void *lf = memchr(t.data() + from + w->chunk_bytes, '\n', (size_t)(size - from - w->chunk_bytes));
                if (lf) end = (const char *)lf - t.data() + 1;
            }
        }
        if (end < 0) break;
        rc = bo_take_chunk(w, t.data() + from, end - from);
        if (rc) break;
        from = end;
    }
    t.erase(t.begin(), t.begin() + from);
    return rc;
}

extern "C" int32_t mpn_bam_out_add_text(mpn_bam_out *w, const char *text, int64_t len) {
    if (!w || len < 0 || (len > 0 && !text) || w->finished) { set_error("mpn_bam_out_add_text: bad arguments"); return -1; }
    if (w->refused_status) return 1;
    try {
        w->pending.insert(w->pending.end(), text, text + len);
        return bo_drain(w, false);
    } catch (const std::bad_alloc &) {
        set_error("mpn_bam_out_add_text: out of host memory");
        return -1;
    }
}

static int64_t bo_finish(mpn_bam_out *w, const uint8_t *header, int64_t header_len, const char *bam_path, const char *bai_path) {
    hipStream_t st = 0;
    const int64_t n = (int64_t)w->size.size();
    // sort: (tid or 2^40, POS, strand), stable, on the device
    std::vector<int64_t> order((size_t)n);
    {
        const Clock c;
        std::vector<uint64_t> hi((size_t)n), lo((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            hi[(size_t)i] = w->tid[(size_t)i] >= 0 ? (uint64_t)w->tid[(size_t)i] : (uint64_t)1 << 40;
            lo[(size_t)i] = ((uint64_t)w->pos0[(size_t)i] + 1) << 1 | (uint64_t)((w->flag[(size_t)i] >> 4) & 1);
        }
        if (n && mpn_sort_order(n, hi.data(), lo.data(), order.data())) return -1;
        w->ms[ST_SORT] += c.ms();
    }
    // cut
    const Clock c_cut;
    BoCut cut;
    const uint64_t voff_first = cut.header(header_len);
    std::vector<uint64_t> voff((size_t)n);
    std::vector<int64_t> start((size_t)n + 1), src((size_t)n);
    std::vector<int32_t> s_tid((size_t)n), s_pos((size_t)n), s_end((size_t)n);
    std::vector<uint8_t> s_mapped((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const size_t i = (size_t)order[(size_t)k];
        start[(size_t)k] = cut.pos;
        voff[(size_t)k] = cut.record(w->size[i]);
        src[(size_t)k] = w->src[i];
        s_tid[(size_t)k] = w->tid[i]; s_pos[(size_t)k] = w->pos0[i]; s_end[(size_t)k] = w->end0[i];
        s_mapped[(size_t)k] = !(w->flag[i] & 4);
    }
    start[(size_t)n] = cut.pos;
    const uint64_t voff_end = cut.close();
    const int64_t n_blocks = cut.n_blocks();
    w->ms[ST_CUT_BAI] += c_cut.ms();

    DevBuf<uint8_t> d_header, d_pay;
    DevBuf<int64_t> d_start, d_src, d_po;
    if (d_header.upload(header, (size_t)header_len, st) || d_start.upload(start.data(), (size_t)n + 1, st) || d_src.upload(src.data(), (size_t)n, st)) return -1;
    FILE *f = fopen(bam_path, "wb");
    if (!f) { set_error("mpn_bam_out_finish: cannot open %s", bam_path); return -1; }
    struct Close { FILE *f; ~Close() { if (f) fclose(f); } } closer{f};
    std::vector<int64_t> addr((size_t)n_blocks + 1, 0), out_off;
    std::vector<uint8_t> host;
    constexpr int64_t ROUND = 1024;               // blocks per round: 64 MiB of payload at the most
    for (int64_t b0 = 0; b0 < n_blocks; b0 += ROUND) {
        const int64_t nb = std::min(ROUND, n_blocks - b0), s0 = cut.block_start[(size_t)b0], s1 = cut.block_start[(size_t)(b0 + nb)];
        DevTimer tm;
        if (d_pay.alloc((size_t)((s1 - s0 + 15) / 16 * 16)) || d_po.upload(cut.block_start.data() + b0, (size_t)nb + 1, st) || tm.start(st)) return -1;
        hipLaunchKernelGGL(bo_gather_kernel, dim3(grid_for(s1 - s0)), dim3(G16_THREADS), 0, st, (const uint8_t *)d_header.p, header_len, (const int64_t *)d_start.p,
                           (const int64_t *)d_src.p, n, (const uint8_t *)w->pool.p, s0, s1, (uint4 *)d_pay.p);
        MPN_HIP_CHECK(hipGetLastError());
        if (tm.stop(st)) return -1;
        BgzfWork work;
        out_off.resize((size_t)nb + 1);
        const int64_t total = bgzf_deflate_resident(d_pay.p, s1 - s0, d_po.p, nb, MPN_BGZF_AUTO, st, work, out_off.data());
        if (total < 0) return -1;
        double ms = 0;
        if (tm.elapsed_ms(&ms)) return -1;
        w->ms[ST_GATHER] += ms;
        DevTimer tm_pack;
        if (bgzf_pack_resident(d_po.p, nb, total, st, work, tm_pack)) return -1;
        MPN_HIP_CHECK(hipStreamSynchronize(st));
        if (tm_pack.elapsed_ms(&ms)) return -1;
        double deflate_ms = 0;
        mpn_bgzf_last_device_ms(&deflate_ms, nullptr);
        w->ms[ST_DEFLATE] += deflate_ms + ms;
        const Clock c_down;
        host.resize((size_t)total);
        if (work.out.download(host.data(), (size_t)total, st)) return -1;
        MPN_HIP_CHECK(hipStreamSynchronize(st));
        w->ms[ST_DOWNLOAD] += c_down.ms();
        const Clock c_file;
        if (fwrite(host.data(), 1, (size_t)total, f) != (size_t)total) { set_error("mpn_bam_out_finish: short write to %s", bam_path); return -1; }
        w->ms[ST_FILE] += c_file.ms();
        for (int64_t k = 0; k < nb; ++k) addr[(size_t)(b0 + k + 1)] = addr[(size_t)b0] + out_off[(size_t)k + 1];
    }
    {
        static const uint8_t eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const Clock c_file;
        if (fwrite(eof, 1, 28, f) != 28 || fclose(f) != 0) { closer.f = nullptr; set_error("mpn_bam_out_finish: short write to %s", bam_path); return -1; }
        closer.f = nullptr;
        w->ms[ST_FILE] += c_file.ms();
    }
    if (bai_path) {
        const Clock c_bai;
        for (int64_t k = 0; k < n; ++k) voff[(size_t)k] = bo_resolve(voff[(size_t)k], addr.data());
        const std::vector<uint8_t> bai = bai_build(w->n_ref, n, s_tid.data(), s_pos.data(), s_end.data(), voff.data(), s_mapped.data(),
                                                   bo_resolve(voff_first, addr.data()), bo_resolve(voff_end, addr.data()));
        w->ms[ST_CUT_BAI] += c_bai.ms();
        const Clock c_file;
        FILE *g = fopen(bai_path, "wb");
        if (!g) { set_error("mpn_bam_out_finish: cannot open %s", bai_path); return -1; }
        const bool ok = fwrite(bai.data(), 1, bai.size(), g) == bai.size();
        if (fclose(g) != 0 || !ok) { set_error("mpn_bam_out_finish: short write to %s", bai_path); return -1; }
        w->ms[ST_FILE] += c_file.ms();
    }
    return n;
}

extern "C" int64_t mpn_bam_out_finish(mpn_bam_out *w, const uint8_t *header, int64_t header_len, const char *bam_path, const char *bai_path) {
    if (!w || !header || header_len < 1 || !bam_path || w->finished) { set_error("mpn_bam_out_finish: bad arguments"); return -2; }
    try {
        if (!w->refused_status) {
            const int rc = bo_drain(w, true);
            if (rc < 0) return -1;
        }
        if (w->refused_status) return -4;
        w->finished = true;
        return bo_finish(w, header, header_len, bam_path, bai_path);
    } catch (const std::bad_alloc &) {
        set_error("mpn_bam_out_finish: out of host memory");
        return -1;
    }
}
