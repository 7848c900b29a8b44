// The walk of a wave over a read's CIGAR, 64 operations per step: shared by csrc/tensor_kernels.hip (the tensors) and
// csrc/clair_call_kernels.hip (the indel events of a pile-up column).  Device only.
#pragma once
#include "mpn_common.h"
#include "tensor_core.h"

namespace mpn {

using namespace mpn_tens;

__device__ __forceinline__ int64_t tens_scan64(int64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// f(k, op, n, r0, q0) in every lane, for the operations of the steps (64 operations each) that can say something about the
// reference positions from .. to: the steps that end before `from` are skipped, the walk stops at the first that starts behind
// `to`.  k: the index of the lane's operation (a lane behind the last operation gets a pad of length 0).  SKIP_ADVANCES: an N
// moves the reference position as htslib's pile-up has it; Clair's scripts do not move over it.  False if an operation code is
// above 8.  Everything that decides a branch around a shuffle is the same in all lanes of the wave.
template <bool SKIP_ADVANCES, class F>
__device__ __forceinline__ bool tens_wave_ops_k(const uint8_t *__restrict__ text, const TensLayout &L, int64_t pos, int64_t from, int64_t to, int lane, F f) {
    int64_t rbase = pos, qbase = 0;
    bool good = true;
    for (int32_t k0 = 0; k0 < L.n_cigar && rbase <= to; k0 += 64) {
        const int32_t k = k0 + lane;
        uint32_t op = OP_P, n = 0;
        if (k < L.n_cigar) {
            const uint32_t w = pile_u32(text, L.cigar + 4 * (int64_t)k);
            op = w & 15u; n = w >> 4;
        }
        if (op > 8) { good = false; op = OP_P; n = 0; }
        const bool match = pile_is_match(op);
        const int64_t radv = (match || op == OP_D || (SKIP_ADVANCES && op == OP_N)) ? n : 0, qadv = (match || op == OP_I || op == OP_S) ? n : 0;
        const int64_t rincl = tens_scan64(radv, lane), qincl = tens_scan64(qadv, lane);
        const int64_t r0 = rbase + rincl - radv, q0 = qbase + qincl - qadv;
        rbase += __shfl(rincl, 63);
        qbase += __shfl(qincl, 63);
        if (rbase >= from) f(k, op, (int64_t)n, r0, q0);
    }
    return __ballot(!good) == 0ull;
}

// the same as Clair's scripts walk a read: f(op, n, r0, q0)
template <class F>
__device__ __forceinline__ bool tens_wave_ops(const uint8_t *__restrict__ text, const TensLayout &L, int64_t pos, int64_t from, int64_t to, int lane, F f) {
    return tens_wave_ops_k<false>(text, L, pos, from, to, lane, [&](int32_t, uint32_t op, int64_t n, int64_t r0, int64_t q0) { f(op, n, r0, q0); });
}

}  // namespace mpn
