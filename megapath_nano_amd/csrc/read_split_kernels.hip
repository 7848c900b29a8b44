// The gather behind include/mpn_reads.h: the reads of a packed batch copied into group-contiguous order, the
// device form of the reference's bin/tools/nanosplit.  A pure HBM copy with arbitrary byte alignment on both sides: 2 B of
// traffic per base moved (one read, one write), 4 B with qualities.  The plan it consumes is made in interval_kernels.hip, next to
// the radix sort it uses.
//
// A wave owns an aligned MPN_SPLIT_CHUNK of the OUTPUT, a lane 16 bytes of it, so every store is one full aligned 16-byte vector
// store, every output byte is written exactly once (padding included, as zeros) and two neighbouring reads never share a store.
// Work is bounded in bytes, not reads: a 2 Mbp read is spread over two thousand wave steps.  The reads that cover a chunk are found
// by a wave-uniform search in out_off for the chunk's first and last byte; a lane then searches only between those two.  The
// search, the unaligned 16-byte load and the launch shape are those of gather16.h, shared with the BAM kernels.
#include "gather16.h"

#include <vector>

namespace mpn {

thread_local int64_t tl_split_ns[2] = {0, 0};

struct SgSide { const uint8_t *src; uint8_t *dst; };

// o_dst[j], o_src[j], o_len[j]: where output read j starts in the output, where its bytes start in the source, its length.
// n_sides: 1 (bases) or 2 (bases and qualities, same offsets).  src_pad: the sources' size rounded up to 4: no load goes beyond it.
// The sources are aligned to 16 bytes.
__global__ __launch_bounds__(G16_THREADS) void split_gather_kernel(SgSide s0, SgSide s1, int n_sides, const int64_t *__restrict__ o_dst,
                                                                   const int64_t *__restrict__ o_src, const int32_t *__restrict__ o_len,
                                                                   int64_t n_out, int64_t out_bytes, int64_t src_pad) {
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (out_bytes + MPN_SPLIT_CHUNK - 1) / MPN_SPLIT_CHUNK;
    for (int64_t c = (int64_t)blockIdx.x * G16_WAVES + (threadIdx.x >> 6); c < n_chunks; c += (int64_t)gridDim.x * G16_WAVES) {
        const int64_t c0 = c * MPN_SPLIT_CHUNK;
        const int64_t c1 = (c0 + MPN_SPLIT_CHUNK < out_bytes ? c0 + MPN_SPLIT_CHUNK : out_bytes) - 1;   // the chunk's last byte
        // wave-uniform: the reads that can cover bytes of [c0, c1]
        const int64_t jlo = last_le(o_dst, 0, n_out - 1, c0), jhi = last_le(o_dst, jlo < 0 ? 0 : jlo, n_out - 1, c1);
        const int64_t p = c0 + lane * 16;
        if (p >= out_bytes) continue;   // (out_bytes is a multiple of 16: a lane's 16 bytes are inside or outside as a whole)
        const int64_t j = last_le(o_dst, jlo < 0 ? 0 : jlo, jhi, p);
        int64_t d = 0, l = 0, s = 0;
        if (j >= 0) { d = o_dst[j]; l = o_len[j]; s = o_src[j] + (p - d); }
        const bool whole = j >= 0 && p + 16 <= d + l;   // all 16 bytes inside read j
        const uint32_t sh16 = (uint32_t)(s & 15);
        for (int t = 0; t < n_sides; ++t) {
            const SgSide sd = t ? s1 : s0;
            uint32_t v[4] = {0, 0, 0, 0};
            // (the second vector must end inside the source: host sources are uploaded with padding to a multiple of 4 only)
            if (whole && (sh16 == 0 || (s & ~(int64_t)15) + 32 <= src_pad)) {
                const uint4 x = load16_at((const uint4 *)(sd.src + (s & ~(int64_t)15)), sh16);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
                // a slot that holds the end of a read, the start of one, short reads or padding, or whose second vector would pass
                // the end of the source: byte by byte
                int64_t jj = j;
#pragma unroll 1
                for (int b = 0; b < 16; ++b) {
                    const int64_t q = p + b;
                    jj = last_le(o_dst, jj < 0 ? 0 : jj, jhi, q);
                    uint32_t byte = 0;
                    if (jj >= 0) {
                        const int64_t dd = o_dst[jj];
                        if (q < dd + o_len[jj]) byte = sd.src[o_src[jj] + (q - dd)];
                    }
                    v[b >> 2] |= byte << (8 * (b & 3));
                }
            }
            *(uint4 *)(sd.dst + p) = make_uint4(v[0], v[1], v[2], v[3]);
        }
    }
}

}  // namespace mpn

using namespace mpn;

extern "C" int64_t mpn_reads_split_last_ns(int32_t which) { return which == 0 || which == 1 ? tl_split_ns[which] : -1; }

extern "C" int mpn_reads_split_gather(int32_t n, const void *seqs, const void *quals, int64_t src_bytes, const int64_t *off, const int32_t *len,
                                      int32_t src_on_device, int64_t n_out, const int32_t *out_read, const int64_t *out_off, int64_t out_bytes,
                                      void *d_out_seqs, void *d_out_quals, int64_t d_out_cap, void *h_out_seqs, void *h_out_quals) {
    tl_split_ns[1] = 0;
    if (n < 0 || n_out < 0 || src_bytes < 0 || out_bytes < 0 || out_bytes % MPN_SPLIT_ALIGN || (n > 0 && (!off || !len)) ||
        (n_out > 0 && (!out_read || !out_off || !seqs)) || (out_bytes > 0 && !d_out_seqs) || (quals && out_bytes > 0 && !d_out_quals) ||
        (h_out_quals && !quals)) {
        set_error("mpn_reads_split_gather: bad arguments (counts and sizes >= 0, out_bytes a multiple of %d, no NULL array that is needed)", MPN_SPLIT_ALIGN);
        return -1;
    }
    if (d_out_cap < out_bytes) { set_error("mpn_reads_split_gather: output capacity %lld < out_bytes %lld", (long long)d_out_cap, (long long)out_bytes); return -1; }
    if (((uintptr_t)d_out_seqs | (uintptr_t)d_out_quals) & (MPN_SPLIT_ALIGN - 1)) { set_error("mpn_reads_split_gather: output buffers must be aligned to %d bytes", MPN_SPLIT_ALIGN); return -1; }
    if (src_on_device && (((uintptr_t)seqs | (uintptr_t)quals) & (MPN_SPLIT_ALIGN - 1))) { set_error("mpn_reads_split_gather: device sources must be aligned to %d bytes", MPN_SPLIT_ALIGN); return -1; }
    for (int32_t i = 0; i < n; ++i)
        if (len[i] < 0 || off[i] < 0 || off[i] > src_bytes - len[i]) {
            set_error("mpn_reads_split_gather: read %d outside the source (off %lld, len %d, %lld source bytes)", (int)i, (long long)off[i], (int)len[i], (long long)src_bytes);
            return -1;
        }
    std::vector<int64_t> o_src((size_t)n_out);
    std::vector<int32_t> o_len((size_t)n_out);
    int64_t end = 0;   // where the previous output read ends
    for (int64_t j = 0; j < n_out; ++j) {
        const int32_t r = out_read[j];
        if (r < 0 || r >= n) { set_error("mpn_reads_split_gather: out_read[%lld] = %d outside [0, %d)", (long long)j, (int)r, (int)n); return -1; }
        if (out_off[j] < end || out_off[j] > out_bytes - len[r]) {
            set_error("mpn_reads_split_gather: out_off[%lld] = %lld overlaps its predecessor or leaves [0, %lld)", (long long)j, (long long)out_off[j], (long long)out_bytes);
            return -1;
        }
        end = out_off[j] + len[r];
        o_src[(size_t)j] = off[r];
        o_len[(size_t)j] = len[r];
    }
    if (out_bytes == 0) return 0;

    hipStream_t st = 0;
    const bool with_q = quals != nullptr;
    if (n_out == 0) {   // nothing but padding
        MPN_HIP_CHECK(hipMemsetAsync(d_out_seqs, 0, (size_t)out_bytes, st));
        if (with_q) MPN_HIP_CHECK(hipMemsetAsync(d_out_quals, 0, (size_t)out_bytes, st));
    } else {
        DevBuf<uint8_t> up_s, up_q;   // host sources: uploaded, zero padded to a multiple of 4
        const uint8_t *d_s = (const uint8_t *)seqs, *d_q = (const uint8_t *)quals;
        if (!src_on_device) {
            const size_t padded = ((size_t)src_bytes + 3) & ~(size_t)3;
            if (up_s.alloc(padded + 4) || (with_q && up_q.alloc(padded + 4))) return -1;
            MPN_HIP_CHECK(hipMemsetAsync(up_s.p + (padded - (padded ? 4 : 0)), 0, 4, st));
            if (src_bytes) MPN_HIP_CHECK(hipMemcpyAsync(up_s.p, seqs, (size_t)src_bytes, hipMemcpyHostToDevice, st));
            if (with_q) {
                MPN_HIP_CHECK(hipMemsetAsync(up_q.p + (padded - (padded ? 4 : 0)), 0, 4, st));
                if (src_bytes) MPN_HIP_CHECK(hipMemcpyAsync(up_q.p, quals, (size_t)src_bytes, hipMemcpyHostToDevice, st));
            }
            d_s = up_s.p;
            d_q = up_q.p;
        }
        DevBuf<int64_t> d_dst, d_src;
        DevBuf<int32_t> d_len;
        if (d_dst.upload(out_off, (size_t)n_out, st) || d_src.upload(o_src.data(), (size_t)n_out, st) || d_len.upload(o_len.data(), (size_t)n_out, st)) return -1;
        DevTimer tm;
        if (tm.start(st)) return -1;
        hipLaunchKernelGGL(split_gather_kernel, dim3(grid_for(out_bytes)), dim3(G16_THREADS), 0, st, SgSide{d_s, (uint8_t *)d_out_seqs},
                           SgSide{d_q, (uint8_t *)d_out_quals}, with_q ? 2 : 1, (const int64_t *)d_dst.p, (const int64_t *)d_src.p,
                           (const int32_t *)d_len.p, n_out, out_bytes, (src_bytes + 3) & ~(int64_t)3);
        MPN_HIP_CHECK(hipGetLastError());
        if (tm.stop(st)) return -1;
        MPN_HIP_CHECK(hipStreamSynchronize(st));   // the uploaded sources and the plan arrays must outlive the kernel
        double ms = 0;
        if (tm.elapsed_ms(&ms)) return -1;
        tl_split_ns[1] = (int64_t)(ms * 1e6);
    }
    if (h_out_seqs) MPN_HIP_CHECK(hipMemcpyAsync(h_out_seqs, d_out_seqs, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
    if (h_out_quals) MPN_HIP_CHECK(hipMemcpyAsync(h_out_quals, d_out_quals, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}
