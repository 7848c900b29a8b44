// gzip decompression on the GPU behind include/mpn_ingest.h (mpn_gzip_inflate): the inflate half of RFC 1951 next to the deflate
// half in bgzf_kernels.hip.  A deflate stream is serial, so the parallelism is across streams: one wave (a workgroup of 64 lanes) per
// stream, a stream being a whole file -- its members are decoded one after the other by the same wave.  Workgroups do not talk to
// each other and nothing waits but at __syncthreads.
//
//   lane 0      runs the serial decoder of inflate_core.h (bit reader, code construction, symbol loop, member headers and
//               trailers) into a 32 KiB ring in LDS: back-references read LDS, never global memory this workgroup has written.
//   all lanes   flush the ring whenever 16 KiB are pending or a member ends: 16-byte stores to the stream's slot (as far as the
//               slot's capacity reaches: an overflowing stream is decoded to its end without stores, its exact length is reported),
//               and the CRC-32 of the flushed bytes, a slice per lane joined by x^(8 * bytes behind the slice) mod P
//               (crc32_poly.h, as bgzf_kernels.hip stage E does), folded into the member's register.
//
// LDS per workgroup: 32 KiB ring + 2 x 2.6 KiB codes + 1 KiB CRC table + 0.3 KiB code lengths = 39 448 B (4 workgroups share a
// CU's 160 KiB; below the 64 KiB every runtime grants).  Every loop runs to the stream's remaining input, to
// a flush's length or to a table size; the decode/flush rounds themselves are bounded by inf_max_calls() of the compressed length.
// Streams are launched in descending order of compressed size.
#include "mpn_common.h"
#include "inflate_core.h"

#include <numeric>

namespace mpn {

using namespace mpn_inf;

thread_local double tl_ingest_ms[2] = {0, 0};   // device time of the last calls on this thread: inflate, FASTA scan

constexpr int INF_THREADS = 64;

struct InfShared {
    uint8_t ring[INF_WIN];
    InfCode ll, dc;
    uint32_t crc_tab[256];
    uint8_t lens[INF_MAX_LENS];
    long long flushed, out_pos;
    uint32_t crc;
    int done;
};

// ring[f .. f + L) -> slot[f ..) below cap; returns the CRC register after these bytes.  All lanes call it and get the same value.
// slot is 16-byte aligned, so a byte's place in the slot and in the ring agree mod 16.
__device__ __forceinline__ uint32_t inf_flush_wave(const InfShared &s, int lane, long long f, int L, uint8_t *__restrict__ slot, long long cap,
                                                   uint32_t crc) {
    const int per = (L + INF_THREADS - 1) / INF_THREADS;
    const int a = min(L, lane * per), b = min(L, a + per);
    uint32_t c = 0;
    for (int k = a; k < b; ++k) c = s.crc_tab[(c ^ s.ring[(f + k) & INF_MASK]) & 0xff] ^ (c >> 8);
    uint32_t part = mpn_crc::crc_slice(c, (uint32_t)(L - b));
    for (int off = 32; off >= 1; off >>= 1) part ^= (uint32_t)__shfl_xor((int)part, off);
    const uint32_t out_crc = mpn_crc::crc_join(crc, (uint32_t)L, part);

    const int head = min(L, (int)((16 - (f & 15)) & 15));
    if (lane < head) { const long long p = f + lane; if (p < cap) slot[p] = s.ring[p & INF_MASK]; }
    const int n16 = (L - head) >> 4;
    for (int j = lane; j < n16; j += INF_THREADS) {
        const long long p = f + head + 16 * j;
        if (p + 16 <= cap) *reinterpret_cast<uint4 *>(slot + p) = *reinterpret_cast<const uint4 *>(s.ring + (p & INF_MASK));
        else for (int k = 0; k < 16; ++k) if (p + k < cap) slot[p + k] = s.ring[(p + k) & INF_MASK];
    }
    for (int k = head + 16 * n16 + lane; k < L; k += INF_THREADS) { const long long p = f + k; if (p < cap) slot[p] = s.ring[p & INF_MASK]; }
    return out_crc;
}

__global__ __launch_bounds__(INF_THREADS) void gzip_inflate_kernel(const uint8_t *__restrict__ in, const int64_t *__restrict__ in_off,
                                                                   const int32_t *__restrict__ order, uint8_t *__restrict__ out,
                                                                   const int64_t *__restrict__ slot_off, const int64_t *__restrict__ slot_cap,
                                                                   int64_t *__restrict__ out_len, int32_t *__restrict__ n_members,
                                                                   int32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) InfShared s;
    const int lane = threadIdx.x;
    const int i = order[blockIdx.x];
    const int64_t base = in_off[0];                       // the device copy of the input starts at in_off[0]
    const int64_t in_len = in_off[i + 1] - in_off[i];
    uint8_t *__restrict__ slot = out + slot_off[i];
    const long long cap = slot_cap[i];
    for (int k = lane; k < 256; k += INF_THREADS) s.crc_tab[k] = mpn_crc::crc_entry((uint32_t)k);
    InfState st;
    inf_init(&st, in_off[i] - base, in_off[i + 1] - base);
    __syncthreads();

    bool finished = false;
    const int64_t max_calls = inf_max_calls(in_len);
    for (int64_t it = 0; it < max_calls && !finished; ++it) {
        if (lane == 0) {
            s.done = inf_run(&st, in, s.ring, &s.ll, &s.dc, s.lens);
            s.flushed = st.flushed; s.out_pos = st.out_pos; s.crc = st.crc;
        }
        __syncthreads();
        const long long f = s.flushed;
        const int L = (int)(s.out_pos - f);                // at most INF_HALF + 257
        finished = s.done != 0;
        uint32_t crc = s.crc;
        if (L > 0) crc = inf_flush_wave(s, lane, f, L, slot, cap, crc);
        if (lane == 0) { st.flushed = st.out_pos; st.crc = crc; }
        __syncthreads();                                   // the ring has been read before lane 0 writes on
    }
    if (lane == 0) {
        out_len[i] = st.out_pos;
        n_members[i] = st.members;
        status[i] = finished ? inf_final_status(&st, cap) : MPN_INFLATE_TRUNCATED;
    }
}

}  // namespace mpn

using namespace mpn;

namespace {
int check_args(int64_t n, const int64_t *in_off, const int64_t *slot_off, const int64_t *slot_cap, const void *o1, const void *o2, const void *o3) {
    if (n < 0 || n > 0x7fffffff || !in_off || (n > 0 && (!slot_off || !slot_cap || !o1 || !o2 || !o3))) return -2;
    for (int64_t i = 0; i < n; ++i)
        if (in_off[i + 1] < in_off[i] || slot_off[i] < 0 || (slot_off[i] & 15) || slot_cap[i] < 0) return -2;
    return 0;
}
}  // namespace

extern "C" void mpn_ingest_last_device_ms(double *inflate_ms, double *scan_ms) {
    if (inflate_ms) *inflate_ms = tl_ingest_ms[0];
    if (scan_ms) *scan_ms = tl_ingest_ms[1];
}

extern "C" int32_t mpn_gzip_inflate_device(int64_t n, const void *d_in, const int64_t *in_off, void *d_out, const int64_t *slot_off,
                                           const int64_t *slot_cap, int64_t *out_len, int32_t *n_members, int32_t *status) {
    tl_ingest_ms[0] = 0;
    if (check_args(n, in_off, slot_off, slot_cap, out_len, n_members, status) || ((uintptr_t)d_out & 15)) {
        set_error("mpn_gzip_inflate: bad arguments");
        return -2;
    }
    if (n == 0) return 0;
    if ((in_off[n] > in_off[0] && !d_in) || !d_out) { set_error("mpn_gzip_inflate: bad arguments"); return -2; }
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return in_off[a + 1] - in_off[a] > in_off[b + 1] - in_off[b]; });
    hipStream_t st = 0;
    DevBuf<int64_t> d_io, d_so, d_sc, d_len;
    DevBuf<int32_t> d_ord, d_mem, d_stat;
    DevTimer tm;
    if (d_io.upload(in_off, (size_t)n + 1, st) || d_so.upload(slot_off, (size_t)n, st) || d_sc.upload(slot_cap, (size_t)n, st) ||
        d_ord.upload(order.data(), (size_t)n, st) || d_len.alloc((size_t)n) || d_mem.alloc((size_t)n) || d_stat.alloc((size_t)n) || tm.start(st))
        return -1;
    hipLaunchKernelGGL(gzip_inflate_kernel, dim3((unsigned)n), dim3(INF_THREADS), 0, st, (const uint8_t *)d_in, (const int64_t *)d_io.p,
                       (const int32_t *)d_ord.p, (uint8_t *)d_out, (const int64_t *)d_so.p, (const int64_t *)d_sc.p, d_len.p, d_mem.p, d_stat.p);
    MPN_HIP_CHECK(hipGetLastError());
    if (tm.stop(st)) return -1;
    if (d_len.download(out_len, (size_t)n, st) || d_mem.download(n_members, (size_t)n, st) || d_stat.download(status, (size_t)n, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return tm.elapsed_ms(&tl_ingest_ms[0]);
}

extern "C" int32_t mpn_gzip_inflate(int64_t n, const uint8_t *in, const int64_t *in_off, uint8_t *out, const int64_t *slot_off,
                                    const int64_t *slot_cap, int64_t *out_len, int32_t *n_members, int32_t *status) {
    tl_ingest_ms[0] = 0;
    if (check_args(n, in_off, slot_off, slot_cap, out_len, n_members, status)) { set_error("mpn_gzip_inflate: bad arguments"); return -2; }
    if (n == 0) return 0;
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) total = std::max(total, slot_off[i] + slot_cap[i]);
    const int64_t in_bytes = in_off[n] - in_off[0];
    if ((in_bytes > 0 && !in) || (total > 0 && !out)) { set_error("mpn_gzip_inflate: bad arguments"); return -2; }
    hipStream_t st = 0;
    DevBuf<uint8_t> d_in, d_out;
    if (d_in.upload(in ? in + in_off[0] : nullptr, (size_t)in_bytes, st) || d_out.upload(out, (size_t)total, st)) return -1;
    const int32_t rc = mpn_gzip_inflate_device(n, d_in.p, in_off, d_out.p, slot_off, slot_cap, out_len, n_members, status);
    if (rc) return rc;
    if (d_out.download(out, (size_t)total, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}
