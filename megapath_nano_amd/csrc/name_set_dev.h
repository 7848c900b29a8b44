// The resident form of a name set (name_set_core.h) and the word readers a lane probes it with: shared by
// csrc/name_lookup_kernels.hip (read names in FASTQ text) and csrc/bam_out_kernels.hip (RNAME / RNEXT in SAM text).  Device code.
#pragma once
#include "gather16.h"
#include "name_set_core.h"

struct mpn_name_set {
    mpn::NsSlot *d_table = nullptr;
    uint4 *d_pool = nullptr;
    int64_t slots = 0, n = 0, distinct = 0;
};

namespace mpn {

struct NsTextWords {      // the words of the id at byte o of the aligned vectors base
    const uint4 *__restrict__ base;
    int64_t o;
    int32_t len;
    __device__ __forceinline__ NsWord operator()(uint32_t k) const {
        const int64_t b = o + 16 * (int64_t)k;
        const uint4 *p = base + (b >> 4);
        const uint32_t sh = (uint32_t)(b & 15), left = (uint32_t)len - 16 * k;
        const uint4 v = left >= 16 ? load16_at(p, sh) : load16_head(p, sh, left);
        return NsWord{v.x, v.y, v.z, v.w};
    }
};
struct NsDevPool {
    const uint4 *__restrict__ pool;
    __device__ __forceinline__ NsWord operator()(uint32_t k) const {
        const uint4 v = pool[k];
        return NsWord{v.x, v.y, v.z, v.w};
    }
};

}  // namespace mpn
