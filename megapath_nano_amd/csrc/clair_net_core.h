// What is the same on the device and on the host behind include/mpn_clair.h: the activations, the LSTM cell, the softmax, the
// offsets of the flat host layout, and the index maps of the device layouts (which k an MFMA step of the recurrent kernel takes,
// where a recurrent weight sits in the register image, how L3 and the heads are laid out).  Written from clair/model.py and
// clair/selu.py as DESIGN.md section 6 item 18 restates them.  It compiles for the device (csrc/clair_net_kernels.hip) and for the
// host (scripts/clair_net_host_check.cpp runs one forward pass serially through it, in the device's summation order).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/mpn_clair.h"

#if defined(__HIPCC__)
#define CLAIR_HD __host__ __device__ inline
#else
#define CLAIR_HD inline
#endif

namespace mpn_clair {

constexpr int STEPS = MPN_CLAIR_STEPS, FEATURES = MPN_CLAIR_FEATURES, UNITS = MPN_CLAIR_UNITS, GATES = 4 * UNITS, BI = 2 * UNITS;
constexpr int CELLS = STEPS * FEATURES;                 // 1056 integers of a tensor
constexpr int L3_OUT = 30, L3_FLAT = L3_OUT * BI;       // 7680, index u * 256 + c
constexpr int L4_OUT = 192, L5_OUT = 96, L5_ALL = 4 * L5_OUT, PROBS = MPN_CLAIR_PROBS, N_HEADS = 4;
constexpr int TILE = MPN_CLAIR_TILE;
static_assert(CELLS == 1056 && L3_FLAT == 7680 && PROBS == 21 + 3 + 33 + 33, "the network");

// ---- the flat host layout (mpn_clair.h) ----------------------------------------------------------------------------------------
CLAIR_HD int lstm_inputs(int layer) { return layer == 0 ? FEATURES : BI; }
CLAIR_HD int64_t lstm_block(int layer) { return (int64_t)(lstm_inputs(layer) + UNITS) * GATES + GATES; }      // kernel and bias of a direction
CLAIR_HD int64_t off_lstm_kernel(int layer, int dir) { return (layer ? 2 * lstm_block(0) : 0) + dir * lstm_block(layer); }
CLAIR_HD int64_t off_lstm_bias(int layer, int dir) { return off_lstm_kernel(layer, dir) + (int64_t)(lstm_inputs(layer) + UNITS) * GATES; }
constexpr int64_t OFF_L3_KERNEL = 2 * ((32 + 128) * 512 + 512) + 2 * ((256 + 128) * 512 + 512);     // [c][t][u]
constexpr int64_t OFF_L3_BIAS = OFF_L3_KERNEL + (int64_t)BI * STEPS * L3_OUT;                      // [c][u]
constexpr int64_t OFF_L4_KERNEL = OFF_L3_BIAS + (int64_t)BI * L3_OUT;
constexpr int64_t OFF_L4_BIAS = OFF_L4_KERNEL + (int64_t)L3_FLAT * L4_OUT;
constexpr int64_t OFF_L5 = OFF_L4_BIAS + L4_OUT, L5_BLOCK = (int64_t)L4_OUT * L5_OUT + L5_OUT;
constexpr int64_t OFF_HEADS = OFF_L5 + 4 * L5_BLOCK;
CLAIR_HD int head_width(int h) { return h == 0 ? 21 : h == 1 ? 3 : 33; }
CLAIR_HD int head_begin(int h) { return h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57; }
CLAIR_HD int head_of(int o) { return o < 21 ? 0 : o < 24 ? 1 : o < 57 ? 2 : 3; }
CLAIR_HD int64_t off_head_kernel(int h) {
    int64_t at = OFF_HEADS;
    for (int k = 0; k < h; ++k) at += (int64_t)L5_OUT * head_width(k) + head_width(k);
    return at;
}
CLAIR_HD int64_t off_head_bias(int h) { return off_head_kernel(h) + (int64_t)L5_OUT * head_width(h); }
static_assert(OFF_HEADS + 96 * 90 + 90 == MPN_CLAIR_WEIGHTS, "the flat layout");

// ---- the order of a long sum ---------------------------------------------------------------------------------------------------------
// A product over k is summed in blocks of SUM_BLOCK: every block is one fmaf chain from zero, k ascending, and the blocks are
// added in order.  One chain over the 7680 inputs of L4 would carry the rounding of 7680 dependent additions (measured: 5 x the
// deviation of a blocked float32 sum on the CPU); blocks of 256 carry that of 256 + 30.  Products of at most 256 inputs (both
// LSTM projections, L5, the heads) are a single chain.
constexpr int SUM_BLOCK = 256;
// sum over k < n of x[k] * w[k * stride], in that order
CLAIR_HD float blocked_dot(const float *x, const float *w, int64_t stride, int n) {
    float total = 0.f;
    for (int k0 = 0; k0 < n; k0 += SUM_BLOCK) {
        float acc = 0.f;
        for (int k = k0; k < n && k < k0 + SUM_BLOCK; ++k) acc = fmaf(x[k], w[(int64_t)k * stride], acc);
        total += acc;
    }
    return total;
}

// ---- the recurrent kernel's maps ---------------------------------------------------------------------------------------------------
// A workgroup carries TILE batch rows of one direction; its 8 waves split the 128 units, 16 each, and a wave holds the four gate
// columns of its units, so that i, j, f and o of a (row, unit) land in the same lane.  One 16x16x4 MFMA step s (0 .. 31) takes,
// in its k slot q (0 .. 3), the hidden unit rec_k(q, s): a lane then reads 32 consecutive floats of h.  The chain of a gate is
// therefore: the input projection (with its bias), then s = 0 .. 31, inside a step q = 0 .. 3.
constexpr int REC_WAVES = 8, REC_UNITS = UNITS / REC_WAVES, REC_STEPS = UNITS / 4;
CLAIR_HD int rec_k(int q, int s) { return q * REC_STEPS + s; }
// where W_h[k][gate * 128 + unit] of a direction sits in the image that a wave loads into its registers: [dir][wave][s * 4 + gate][lane]
CLAIR_HD int64_t rec_image_index(int dir, int k, int gate, int unit) {
    const int q = k / REC_STEPS, s = k % REC_STEPS, wave = unit / REC_UNITS, lane = q * 16 + unit % REC_UNITS;
    return (((int64_t)dir * REC_WAVES + wave) * (REC_STEPS * 4) + (s * 4 + gate)) * 64 + lane;
}

// ---- the arithmetic ------------------------------------------------------------------------------------------------------------------
CLAIR_HD float selu(float x) {
    const float alpha = 1.6732632423543772848170429916717f, scale = 1.0507009873554804934193349852946f;
    return scale * (x >= 0.0f ? x : alpha * (expf(x) - 1.0f));
}
CLAIR_HD float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// c' = c s(f) + s(i) tanh(j); h' = tanh(c') s(o)   (forget_bias 0, no peephole, no clipping)
CLAIR_HD float lstm_cell(float i, float j, float f, float o, float *c) {
    const float c1 = *c * sigmoid(f) + sigmoid(i) * tanhf(j);
    *c = c1;
    return tanhf(c1) * sigmoid(o);
}
// entry i of the softmax over v[0 .. n): the maximum, then the sum in index order
CLAIR_HD float softmax_at(const float *v, int n, int i) {
    float m = v[0];
    for (int k = 1; k < n; ++k) m = v[k] > m ? v[k] : m;
    float sum = 0.0f;
    for (int k = 0; k < n; ++k) sum += expf(v[k] - m);
    return expf(v[i] - m) / sum;
}

}  // namespace mpn_clair
