// Runs one forward pass of Clair's network on the CPU, serially, through megapath_nano_amd/csrc/clair_net_core.h -- the activations,
// the cell, the softmax, the offsets of the flat layout and the index maps of the device layouts, with every sum in the order the
// kernels of csrc/clair_net_kernels.hip take it -- so that the layouts have been through the host's tools before they meet a GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -o clair_net_host_check scripts/clair_net_host_check.cpp
//   clair_net_host_check weights.bin tensors.bin results.bin
//
// weights.bin: MPN_CLAIR_WEIGHTS float32 in the flat layout of include/mpn_clair.h.  tensors.bin: u32 n, then n x 1056 int32.
// results.bin: per tensor the float32 of LSTM1 (33 x 256), LSTM2 (33 x 256), L3 (7680), L4 (192) and the 90 probabilities.
// Every array is a heap block of its exact size: a read outside it is reported.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../megapath_nano_amd/csrc/clair_net_core.h"

using namespace mpn_clair;

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// one bidirectional layer for one tensor: x [33][n_in] -> out [33][256]
static void lstm_layer(const std::vector<float> &weights, int layer, const std::vector<float> &x, std::vector<float> &out) {
    const int n_in = lstm_inputs(layer);
    // the register image of the recurrent kernel, built by the same map the device upload uses
    std::vector<float> image((size_t)2 * UNITS * GATES);
    for (int dir = 0; dir < 2; ++dir)
        for (int k = 0; k < UNITS; ++k)
            for (int gate = 0; gate < 4; ++gate)
                for (int unit = 0; unit < UNITS; ++unit)
                    image[(size_t)rec_image_index(dir, k, gate, unit)] = weights[(size_t)off_lstm_kernel(layer, dir) + (size_t)(n_in + k) * GATES + gate * UNITS + unit];
    for (int dir = 0; dir < 2; ++dir) {
        const float *kernel = &weights[(size_t)off_lstm_kernel(layer, dir)], *bias = &weights[(size_t)off_lstm_bias(layer, dir)];
        std::vector<float> h(UNITS, 0.f), h1(UNITS, 0.f), c(UNITS, 0.f);
        for (int step = 0; step < STEPS; ++step) {
            const int t = dir ? STEPS - 1 - step : step;
            for (int unit = 0; unit < UNITS; ++unit) {
                float g[4];
                for (int gate = 0; gate < 4; ++gate) {
                    // the projection, then the bias
                    float acc = blocked_dot(&x[(size_t)t * n_in], kernel + gate * UNITS + unit, GATES, n_in) + bias[gate * UNITS + unit];
                    const int wave = unit / REC_UNITS;
                    for (int s = 0; s < REC_STEPS; ++s)     // the recurrence: an MFMA step at a time, its four k slots in order
                        for (int q = 0; q < 4; ++q) {
                            const size_t at = (((size_t)dir * REC_WAVES + wave) * (REC_STEPS * 4) + (s * 4 + gate)) * 64 + q * 16 + unit % REC_UNITS;
                            acc = fmaf(h[rec_k(q, s)], image[at], acc);
                        }
                    g[gate] = acc;
                }
                h1[unit] = lstm_cell(g[0], g[1], g[2], g[3], &c[unit]);
                out[(size_t)t * BI + dir * UNITS + unit] = h1[unit];
            }
            h.swap(h1);
        }
    }
}

static void dense_selu(const float *x, int n_in, const float *kernel, const float *bias, int n_out, float *out) {
    for (int j = 0; j < n_out; ++j) out[j] = selu(blocked_dot(x, kernel + j, n_out, n_in) + bias[j]);
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s weights.bin tensors.bin results.bin\n", argv[0]); return 2; }
    FILE *fw = fopen(argv[1], "rb"), *fi = fopen(argv[2], "rb"), *fo = fopen(argv[3], "wb");
    if (!fw || !fi || !fo) { perror("open"); return 2; }
    std::vector<float> weights(MPN_CLAIR_WEIGHTS);
    uint32_t n = 0;
    if (!read_exact(fw, weights.data(), weights.size() * sizeof(float)) || fgetc(fw) != EOF || !read_exact(fi, &n, 4)) {
        fprintf(stderr, "the weights are not %d floats, or the tensor file is short\n", MPN_CLAIR_WEIGHTS);
        return 2;
    }
    for (uint32_t b = 0; b < n; ++b) {
        std::vector<int32_t> cells(CELLS);
        if (!read_exact(fi, cells.data(), CELLS * sizeof(int32_t))) { fprintf(stderr, "short tensor file\n"); return 2; }
        std::vector<float> x(CELLS), lstm1((size_t)STEPS * BI), lstm2((size_t)STEPS * BI), l3(L3_FLAT), l4(L4_OUT), l5(L5_OUT), y(PROBS), probs(PROBS);
        for (int i = 0; i < CELLS; ++i) x[i] = (float)cells[i];       // [step][row * 4 + channel]: the tensor as it lies
        lstm_layer(weights, 0, x, lstm1);
        lstm_layer(weights, 1, lstm1, lstm2);
        for (int c = 0; c < BI; ++c)
            for (int u = 0; u < L3_OUT; ++u) {
                float acc = 0.f;
                for (int t = 0; t < STEPS; ++t) acc = fmaf(lstm2[(size_t)t * BI + c], weights[(size_t)OFF_L3_KERNEL + ((size_t)c * STEPS + t) * L3_OUT + u], acc);
                l3[(size_t)u * BI + c] = selu(acc + weights[(size_t)OFF_L3_BIAS + (size_t)c * L3_OUT + u]);
            }
        dense_selu(l3.data(), L3_FLAT, &weights[(size_t)OFF_L4_KERNEL], &weights[(size_t)OFF_L4_BIAS], L4_OUT, l4.data());
        for (int h = 0; h < N_HEADS; ++h) {
            const float *k5 = &weights[(size_t)(OFF_L5 + h * L5_BLOCK)];
            dense_selu(l4.data(), L4_OUT, k5, k5 + (size_t)L4_OUT * L5_OUT, L5_OUT, l5.data());
            dense_selu(l5.data(), L5_OUT, &weights[(size_t)off_head_kernel(h)], &weights[(size_t)off_head_bias(h)], head_width(h), &y[head_begin(h)]);
        }
        for (int o = 0; o < PROBS; ++o) {
            const int h = head_of(o);
            probs[o] = softmax_at(&y[head_begin(h)], head_width(h), o - head_begin(h));
        }
        const std::vector<float> *parts[5] = {&lstm1, &lstm2, &l3, &l4, &probs};
        for (const std::vector<float> *p : parts)
            if (fwrite(p->data(), sizeof(float), p->size(), fo) != p->size()) { perror("write"); return 2; }
    }
    if (fclose(fo) != 0) { perror("close"); return 2; }
    fclose(fw);
    fclose(fi);
    return 0;
}
