// What the chunked byte gathers share: split_gather_kernel (read_split_kernels.hip), bam_flatten_kernel and bam_decode_kernel
// (bam_in_kernels.hip).  A wave owns an aligned chunk of 64 x 16 bytes of the OUTPUT, a lane 16 bytes of it: every store is one
// aligned 16-byte store and every output byte is written once.  The work is bounded in bytes: a grid of at most G16_MAX_BLOCKS
// workgroups takes the chunks in rounds.  The pieces that cover a chunk are found by binary search in their ascending starts.
#pragma once
#include "mpn_common.h"
#include "../../include/mpn_ingest.h"
#include "../../include/mpn_reads.h"

namespace mpn {

constexpr int G16_THREADS = 256, G16_WAVES = G16_THREADS / 64;
constexpr int G16_MAX_BLOCKS = 256 * 8;   // 8 resident blocks of 256 threads on each of 256 CUs; more output is taken in further rounds
constexpr int G16_CHUNK = 64 * 16;        // a wave step is 64 lanes x 16 bytes
static_assert(MPN_SPLIT_CHUNK == G16_CHUNK && MPN_BAM_CHUNK == G16_CHUNK, "the chunk the headers promise is a wave step");

inline int grid_for(int64_t out_bytes) {
    const int64_t n_chunks = (out_bytes + G16_CHUNK - 1) / G16_CHUNK;
    return (int)std::max<int64_t>(1, std::min<int64_t>((n_chunks + G16_WAVES - 1) / G16_WAVES, G16_MAX_BLOCKS));
}

// last j in [lo, hi] with v[j] <= q, or lo - 1 if there is none (v ascending; equal entries are pieces of length 0)
__device__ __forceinline__ int64_t last_le(const int64_t *__restrict__ v, int64_t lo, int64_t hi, int64_t q) {
    int64_t a = lo, b = hi + 1;   // answer in [a - 1, b - 1]
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (v[mid] <= q) a = mid + 1; else b = mid;
    }
    return a - 1;
}

// The 16 bytes that start sh16 (0..15) bytes into the aligned vector v[0], by the one or two aligned 16-byte vectors that hold
// them, shifted into place; the second vector is touched only when its bytes are needed.  Both vectors hold at least one of the
// 16 bytes, so they lie in the allocation the bytes lie in (device allocations are 16-byte granular); a caller whose source may
// end sooner checks that itself.
// (load16_first: the same with only the first cnt of the 16 bytes wanted, so that the second vector is touched only when one of
// THOSE lies in it; what the other bytes of the result are is not defined.)
__device__ __forceinline__ uint4 load16_first(const uint4 *v, uint32_t sh16, uint32_t cnt) {
    const uint4 lo4 = v[0], hi4 = sh16 + cnt > 16 ? v[1] : make_uint4(0, 0, 0, 0);
    uint32_t x0, x1, x2, x3, x4;
    switch (sh16 >> 2) {   // (the same in every lane that copies from the same piece)
        case 0: x0 = lo4.x; x1 = lo4.y; x2 = lo4.z; x3 = lo4.w; x4 = hi4.x; break;
        case 1: x0 = lo4.y; x1 = lo4.z; x2 = lo4.w; x3 = hi4.x; x4 = hi4.y; break;
        case 2: x0 = lo4.z; x1 = lo4.w; x2 = hi4.x; x3 = hi4.y; x4 = hi4.z; break;
        default: x0 = lo4.w; x1 = hi4.x; x2 = hi4.y; x3 = hi4.z; x4 = hi4.w; break;
    }
    const uint32_t sh = sh16 & 3;
    return make_uint4(__builtin_amdgcn_alignbyte(x1, x0, sh), __builtin_amdgcn_alignbyte(x2, x1, sh), __builtin_amdgcn_alignbyte(x3, x2, sh),
                      __builtin_amdgcn_alignbyte(x4, x3, sh));
}
__device__ __forceinline__ uint4 load16_at(const uint4 *v, uint32_t sh16) { return load16_first(v, sh16, 16); }
// The first cnt (1..15) of those 16 bytes and zeros behind them: for the end of a piece that has no 16 bytes left.  Both vectors
// that are touched hold a byte of the piece here too.
__device__ __forceinline__ uint4 load16_head(const uint4 *v, uint32_t sh16, uint32_t cnt) {
    const uint4 w = load16_first(v, sh16, cnt);
    const uint32_t full = cnt >> 2, part = (1u << (8 * (cnt & 3))) - 1;     // whole words kept, the mask of the word behind them
    return make_uint4(full > 0 ? w.x : part & w.x, full > 1 ? w.y : (full == 1 ? part & w.y : 0), full > 2 ? w.z : (full == 2 ? part & w.z : 0),
                      full == 3 ? part & w.w : 0);
}
// 16 bytes from any address.  (A caller that has its source as an aligned base and an offset calls load16_at with them: the
// compiler then still knows that the base is global memory, which an address that went through an integer no longer says.)
__device__ __forceinline__ uint4 load16(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p;
    return load16_at((const uint4 *)(a & ~(uintptr_t)15), (uint32_t)(a & 15));
}

}  // namespace mpn
