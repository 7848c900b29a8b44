// Clair's network (clair/model.py, 2BiLSTM, inference) on resident tensors, behind include/mpn_clair.h.  The rules are DESIGN.md
// section 6 item 18; the arithmetic and the index maps shared with the host are csrc/clair_net_core.h.  Every matrix product is
// float32 on the f32-input MFMA: a k-ordered fmaf chain per output, so a tensor's numbers do not depend on its neighbours.
//
//   clair_gemm_kernel   C = act(A B + bias): a 128 x 64 tile per workgroup of 4 waves, 32 x 64 per wave as two 32x32x2 accumulators,
//                       A and B through LDS in k slices of 32 with the next slice already in registers.  A is int32 for the first
//                       projection (the tensors as mpn_tensor_fill left them) and float32 otherwise.  It runs the input
//                       projections of both LSTM layers (all 33 steps and both directions are one product), L4, and the four L5
//                       layers as one product of 384 columns.  Rows from M on are read as zero and never written.
//   clair_rec_kernel    a workgroup per (direction, MPN_CLAIR_TILE batch rows), 8 waves.  W_h of the direction lives in registers,
//                       128 per lane: a wave holds the four gate columns of 16 units.  Per step, h of the tile is read from LDS as
//                       the A operand of 16x16x4 MFMAs (4 gates = 4 independent accumulators, started from the projection), the
//                       lane that ends up with i, j, f, o of a (row, unit) updates c in its registers and writes h to LDS and to
//                       HBM.  The two 16-row blocks of a tile are separate recurrences: the MFMA chain of one is issued beside the
//                       cells (expf, tanhf) of the other, a barrier per half step.  The projection of the next half step is
//                       fetched before the MFMA chain of this one.
//   clair_l3_kernel     the slice dense: 256 products of (33 -> 30) per tensor, a thread per channel, four tensors per workgroup.
//                       These are separate tiny products over a strided operand; the f32 MFMA has the rate of the vector unit, so
//                       they are plain fmaf chains in step order (the same numbers an MFMA would give).
//   clair_heads_kernel  the four output layers (96 -> 21, 3, 33, 33), selu, and the softmaxes; a thread per output.
#include <memory>
#include <mutex>
#include <set>
#include <stdlib.h>

#include "mpn_common.h"
#include "clair_net_core.h"

namespace mpn {

using namespace mpn_clair;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

static thread_local double tl_clair_ms[6] = {0, 0, 0, 0, 0, 0};     // project, recurrent, l3, l4, heads, total

// ---- the tiled product -------------------------------------------------------------------------------------------------------------
constexpr int GM = 128, GN = 64, GK = 32, GA_LD = GK + 1, GB_LD = GN + 32;

__device__ __forceinline__ f32x4 clair_load4(const float *p) { return *(const f32x4 *)p; }
__device__ __forceinline__ f32x4 clair_load4(const int32_t *p) {
    const int4 v = *(const int4 *)p;
    return f32x4{(float)v.x, (float)v.y, (float)v.z, (float)v.w};
}

// A [M][K] (lda = K), B [K][N], C [M][N]; K a multiple of 32, N of 64 (the host checks), rows of A 16-byte aligned.
template <typename AT, bool SELU>
__global__ __launch_bounds__(256) void clair_gemm_kernel(const AT *__restrict__ A, int64_t M, int K, const float *__restrict__ B, int N,
                                                         const float *__restrict__ bias, float *__restrict__ C) {
    __shared__ float s_a[GM * GA_LD];
    __shared__ __attribute__((aligned(16))) float s_b[GK * GB_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
    const int64_t m0 = (int64_t)blockIdx.y * GM;
    const int n0 = blockIdx.x * GN;
    f32x4 ra[4], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, row = idx >> 3, kq = idx & 7;
            ra[i] = m0 + row < M ? clair_load4(A + (m0 + row) * (int64_t)K + k0 + kq * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i, kr = idx >> 4, c4 = idx & 15;
            rb[i] = clair_load4(B + (int64_t)(k0 + kr) * N + n0 + c4 * 4);
        }
    };
    f32x16 acc0, acc1, sum0, sum1;                           // the chain of a block of SUM_BLOCK, and the blocks before it
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; sum0[r] = 0.f; sum1[r] = 0.f; }
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += GK) {
        __syncthreads();                                     // the slice before this one has been read
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, row = idx >> 3, kq = idx & 7;
#pragma unroll
            for (int j = 0; j < 4; ++j) s_a[row * GA_LD + kq * 4 + j] = ra[i][j];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i, kr = idx >> 4, c4 = idx & 15;
            *(f32x4 *)&s_b[kr * GB_LD + c4 * 4] = rb[i];
        }
        __syncthreads();
        if (k0 + GK < K) fetch(k0 + GK);
        const float *pa = &s_a[(wave * 32 + l32) * GA_LD + half];
        const float *pb = &s_b[half * GB_LD + l32];
#pragma unroll
        for (int s = 0; s < GK / 2; ++s) {                   // k = k0 + 2 s + half: ascending along the chain
            const float a = pa[2 * s], b0 = pb[2 * s * GB_LD], b1 = pb[2 * s * GB_LD + 32];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
        }
        if ((k0 + GK) % SUM_BLOCK == 0 || k0 + GK >= K) {      // blocked_dot's order (clair_net_core.h)
#pragma unroll
            for (int r = 0; r < 16; ++r) { sum0[r] += acc0[r]; sum1[r] += acc1[r]; acc0[r] = 0.f; acc1[r] = 0.f; }
        }
    }
    const int col = n0 + l32;
    const float bias0 = bias[col], bias1 = bias[col + 32];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row < M) {
            const float v0 = sum0[r] + bias0, v1 = sum1[r] + bias1;
            C[row * N + col] = SELU ? selu(v0) : v0;
            C[row * N + col + 32] = SELU ? selu(v1) : v1;
        }
    }
}

// ---- the recurrence ------------------------------------------------------------------------------------------------------------------
constexpr int REC_THREADS = REC_WAVES * 64, REC_LD = UNITS + 4;       // a row of h in LDS: 16-byte aligned, rows 4 banks apart
static_assert(SUM_BLOCK % GK == 0, "a block of the sum is whole slices");
static_assert(TILE == 32 && REC_UNITS == 16 && REC_STEPS == 32, "two 16-row MFMA blocks per tile, 16 units per wave");

// G [rows * 33][1024]: the input projection with its bias, columns dir * 512 + gate * 128 + unit.  image: rec_image_index.
// X [rows rounded up to whole tiles][33][256]: the layer's output, fw | bw.  Rows of the tile from `rows` on: zero projection; their
// h goes to the rows of X that only exist for it (the workspace, never a caller's buffer).
__global__ __launch_bounds__(REC_THREADS) void clair_rec_kernel(const float *__restrict__ G, const float *__restrict__ image, float *__restrict__ X,
                                                                int64_t rows) {
    __shared__ __attribute__((aligned(16))) float s_h[TILE * REC_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, l16 = lane & 15;
    const int dir = blockIdx.y, unit = wave * REC_UNITS + l16;
    const int64_t b0 = (int64_t)blockIdx.x * TILE;
    float w[REC_STEPS * 4];
    const float *img = image + ((int64_t)dir * REC_WAVES + wave) * (REC_STEPS * 4) * 64 + lane;
#pragma unroll
    for (int r = 0; r < REC_STEPS * 4; ++r) w[r] = img[r * 64];
    for (int i = tid; i < TILE * REC_LD; i += REC_THREADS) s_h[i] = 0.f;
    float c0[4], c1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { c0[r] = 0.f; c1[r] = 0.f; }
    // the projection of (step, row block rb): row rb * 16 + q * 4 + reg, the lane's unit, four gates
    auto project = [&](int step, int rb, f32x4 *g) {
        const int t = dir ? STEPS - 1 - step : step;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t b = b0 + rb * 16 + q * 4 + reg;
            const bool valid = b < rows;                     // (a row past the end reads the last row's and takes zero: no branch)
            const float *p = G + ((valid ? b : rows - 1) * STEPS + t) * (int64_t)(2 * GATES) + dir * GATES + unit;
#pragma unroll
            for (int gate = 0; gate < 4; ++gate) {
                const float v = p[gate * UNITS];
                g[gate][reg] = valid ? v : 0.f;
            }
        }
    };
    // the four gates of row block rb: the chain goes on from the projection over h[row][rec_k(q, s)], s = 0 .. 31
    auto chain = [&](int rb, f32x4 *acc) {
        const float *ph = &s_h[(rb * 16 + l16) * REC_LD + q * REC_STEPS];
#pragma unroll
        for (int s4 = 0; s4 < REC_STEPS / 4; ++s4) {
            const f32x4 a = *(const f32x4 *)(ph + 4 * s4);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int gate = 0; gate < 4; ++gate)
                    acc[gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w[(4 * s4 + j) * 4 + gate], acc[gate], 0, 0, 0);
        }
    };
    // the cells of row block rb at `step` from their gates: the result's row q * 4 + reg, column l16
    auto cells = [&](int rb, int step, const f32x4 *g, float *c) {
        const int t = dir ? STEPS - 1 - step : step;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = rb * 16 + q * 4 + reg;
            const float h = lstm_cell(g[0][reg], g[1][reg], g[2][reg], g[3][reg], &c[reg]);
            s_h[row * REC_LD + unit] = h;
            X[((b0 + row) * STEPS + t) * (int64_t)BI + dir * UNITS + unit] = h;       // (X has whole tiles: no branch in the phase)
        }
    };
    // The two row blocks are separate recurrences, so the MFMA chain of one runs beside the cells of the other: a phase reads the
    // rows of h of one block and writes those of the other, and a barrier ends it.  One buffer of h is enough.
    f32x4 acc[4], done[4], next[4];
    project(0, 0, acc);
    project(0, 1, next);
    __syncthreads();
    chain(0, acc);
    __syncthreads();                                         // every wave has read block 0's h before its cells write it
#pragma unroll
    for (int gate = 0; gate < 4; ++gate) { done[gate] = acc[gate]; acc[gate] = next[gate]; }
    for (int step = 0; step + 1 < STEPS; ++step) {
        project(step + 1, 0, next);
        chain(1, acc);                                       // (step, block 1) beside the cells of (step, block 0)
        cells(0, step, done, c0);
        __syncthreads();
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) { done[gate] = acc[gate]; acc[gate] = next[gate]; }
        project(step + 1, 1, next);
        chain(0, acc);                                       // (step + 1, block 0) beside the cells of (step, block 1)
        cells(1, step, done, c1);
        __syncthreads();
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) { done[gate] = acc[gate]; acc[gate] = next[gate]; }
    }
    chain(1, acc);
    cells(0, STEPS - 1, done, c0);
    __syncthreads();                                         // every wave has read block 1's h before its cells write it
    cells(1, STEPS - 1, acc, c1);
}

// ---- L3 ------------------------------------------------------------------------------------------------------------------------------
constexpr int L3_ROWS = 4, L3_GROUP = 10;
static_assert(L3_OUT % L3_GROUP == 0, "the outputs of a unit in groups");

// X [rows][33][256]; kernel [t][u][c], bias [u][c]; out [rows][u * 256 + c]
__global__ __launch_bounds__(BI) void clair_l3_kernel(const float *__restrict__ X, const float *__restrict__ kernel, const float *__restrict__ bias,
                                                      float *__restrict__ out, int64_t rows) {
    const int c = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * L3_ROWS;
    for (int u0 = 0; u0 < L3_OUT; u0 += L3_GROUP) {
        float acc[L3_ROWS][L3_GROUP];
#pragma unroll
        for (int r = 0; r < L3_ROWS; ++r)
#pragma unroll
            for (int u = 0; u < L3_GROUP; ++u) acc[r][u] = 0.f;
        for (int t = 0; t < STEPS; ++t) {
            float x[L3_ROWS];
#pragma unroll
            for (int r = 0; r < L3_ROWS; ++r) x[r] = b0 + r < rows ? X[((b0 + r) * STEPS + t) * (int64_t)BI + c] : 0.f;
#pragma unroll
            for (int u = 0; u < L3_GROUP; ++u) {
                const float wv = kernel[(t * L3_OUT + u0 + u) * BI + c];
#pragma unroll
                for (int r = 0; r < L3_ROWS; ++r) acc[r][u] = fmaf(x[r], wv, acc[r][u]);
            }
        }
#pragma unroll
        for (int r = 0; r < L3_ROWS; ++r)
            if (b0 + r < rows)
#pragma unroll
                for (int u = 0; u < L3_GROUP; ++u) out[(b0 + r) * (int64_t)L3_FLAT + (u0 + u) * BI + c] = selu(acc[r][u] + bias[(u0 + u) * BI + c]);
    }
}

// ---- the output layers -------------------------------------------------------------------------------------------------------------
constexpr int HEAD_THREADS = 128, HEAD_ROWS = 8;

// L5 [rows][4 x 96]; kernel [96][90]: the columns of the four heads side by side; probs [rows][90]
__global__ __launch_bounds__(HEAD_THREADS) void clair_heads_kernel(const float *__restrict__ L5, const float *__restrict__ kernel,
                                                                   const float *__restrict__ bias, float *__restrict__ probs, int64_t rows) {
    __shared__ float s_x[L5_ALL], s_y[PROBS];
    const int o = threadIdx.x, head = head_of(o < PROBS ? o : 0);
    for (int r = 0; r < HEAD_ROWS; ++r) {
        const int64_t b = (int64_t)blockIdx.x * HEAD_ROWS + r;
        if (b >= rows) break;                                // (the whole workgroup)
        for (int i = threadIdx.x; i < L5_ALL; i += HEAD_THREADS) s_x[i] = L5[b * L5_ALL + i];
        __syncthreads();
        if (o < PROBS) {
            float acc = 0.f;
            for (int k = 0; k < L5_OUT; ++k) acc = fmaf(s_x[head * L5_OUT + k], kernel[k * PROBS + o], acc);
            s_y[o] = selu(acc + bias[o]);
        }
        __syncthreads();
        if (o < PROBS) probs[b * PROBS + o] = softmax_at(s_y + head_begin(head), head_width(head), o - head_begin(head));
        __syncthreads();
    }
}

// ---- the model -----------------------------------------------------------------------------------------------------------------------
struct ClairModel {
    int64_t chunk = 0;
    float *wx[2] = {nullptr, nullptr}, *bx[2] = {nullptr, nullptr}, *image[2] = {nullptr, nullptr};       // per LSTM layer
    float *k3 = nullptr, *b3 = nullptr, *k4 = nullptr, *b4 = nullptr, *k5 = nullptr, *b5 = nullptr, *kh = nullptr, *bh = nullptr;
    float *G = nullptr, *X1 = nullptr, *X2 = nullptr, *L3 = nullptr, *L4 = nullptr, *L5 = nullptr;          // the workspace of a chunk
    hipEvent_t ev[9] = {};
    std::vector<void *> owned;
    ~ClairModel() {
        for (void *p : owned) (void)hipFree(p);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
    int put(float **d, const std::vector<float> &h) {
        MPN_HIP_CHECK(hipMalloc((void **)d, h.size() * sizeof(float)));
        owned.push_back(*d);
        MPN_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
    int room(float **d, size_t count) {
        if (guarded_malloc((void **)d, count * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("mpn_clair_model_create: no room for %zu bytes of workspace (MPN_CLAIR_CHUNK = %lld)", count * sizeof(float), (long long)chunk);
            return -1;
        }
        owned.push_back(*d);
        return 0;
    }
};

static std::mutex g_clair_mutex;
static std::set<void *> g_clair_models;

static ClairModel *clair_live(void *handle) {
    std::lock_guard<std::mutex> lock(g_clair_mutex);
    return handle && g_clair_models.count(handle) ? (ClairModel *)handle : nullptr;
}

template <typename AT, bool SELU>
static int clair_gemm(hipStream_t st, const AT *A, int64_t M, int K, const float *B, int N, const float *bias, float *C) {
    if (K % GK || N % GN || M <= 0 || (M + GM - 1) / GM > 0x7fffffff) {
        set_error("mpn_clair_forward: a product of %lld x %d x %d does not fit the tiles", (long long)M, K, N);
        return -1;
    }
    hipLaunchKernelGGL((clair_gemm_kernel<AT, SELU>), dim3((unsigned)(N / GN), (unsigned)((M + GM - 1) / GM)), dim3(256), 0, st, A, M, K, B, N, bias, C);
    MPN_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace mpn

using namespace mpn;

extern "C" int32_t mpn_clair_tile(void) { return MPN_CLAIR_TILE; }

extern "C" void mpn_clair_last_device_ms(double *project_ms, double *recurrent_ms, double *l3_ms, double *l4_ms, double *heads_ms, double *total_ms) {
    double *out[6] = {project_ms, recurrent_ms, l3_ms, l4_ms, heads_ms, total_ms};
    for (int i = 0; i < 6; ++i)
        if (out[i]) *out[i] = tl_clair_ms[i];
}

extern "C" int32_t mpn_clair_model_create(const float *weights, int64_t count, void **handle) {
    if (!weights || !handle || count != MPN_CLAIR_WEIGHTS) {
        set_error("mpn_clair_model_create: bad arguments (%lld weights, %d are expected)", (long long)count, MPN_CLAIR_WEIGHTS);
        return -2;
    }
    *handle = nullptr;
    int64_t chunk = MPN_CLAIR_CHUNK_DEFAULT;
    if (const char *e = getenv("MPN_CLAIR_CHUNK")) {
        char *end = nullptr;
        const long long v = strtoll(e, &end, 10);
        if (end == e || *end || v < 1 || v > MPN_CLAIR_CHUNK_MAX) {
            set_error("mpn_clair_model_create: MPN_CLAIR_CHUNK=%s is not a number of 1 .. %d", e, MPN_CLAIR_CHUNK_MAX);
            return -2;
        }
        chunk = v;
    }
    std::unique_ptr<ClairModel> m(new ClairModel);
    m->chunk = chunk;
    // ---- the variables in the layouts of the kernels
    for (int layer = 0; layer < 2; ++layer) {
        const int n_in = lstm_inputs(layer);
        std::vector<float> wx((size_t)n_in * 2 * GATES), bx(2 * GATES), image((size_t)2 * UNITS * GATES);
        for (int dir = 0; dir < 2; ++dir) {
            const float *kernel = weights + off_lstm_kernel(layer, dir), *bias = weights + off_lstm_bias(layer, dir);
            for (int k = 0; k < n_in; ++k)
                for (int col = 0; col < GATES; ++col) wx[(size_t)k * 2 * GATES + dir * GATES + col] = kernel[(size_t)k * GATES + col];
            for (int col = 0; col < GATES; ++col) bx[dir * GATES + col] = bias[col];
            for (int k = 0; k < UNITS; ++k)
                for (int gate = 0; gate < 4; ++gate)
                    for (int unit = 0; unit < UNITS; ++unit)
                        image[(size_t)rec_image_index(dir, k, gate, unit)] = kernel[(size_t)(n_in + k) * GATES + gate * UNITS + unit];
        }
        if (m->put(&m->wx[layer], wx) || m->put(&m->bx[layer], bx) || m->put(&m->image[layer], image)) return -1;
    }
    {
        std::vector<float> k3((size_t)STEPS * L3_OUT * BI), b3((size_t)L3_OUT * BI);
        for (int c = 0; c < BI; ++c)
            for (int u = 0; u < L3_OUT; ++u) {
                for (int t = 0; t < STEPS; ++t) k3[((size_t)t * L3_OUT + u) * BI + c] = weights[OFF_L3_KERNEL + ((size_t)c * STEPS + t) * L3_OUT + u];
                b3[(size_t)u * BI + c] = weights[OFF_L3_BIAS + (size_t)c * L3_OUT + u];
            }
        std::vector<float> k4(weights + OFF_L4_KERNEL, weights + OFF_L4_BIAS), b4(weights + OFF_L4_BIAS, weights + OFF_L5);
        std::vector<float> k5((size_t)L4_OUT * L5_ALL), b5(L5_ALL), kh((size_t)L5_OUT * PROBS), bh(PROBS);
        for (int h = 0; h < N_HEADS; ++h) {
            const float *kernel = weights + OFF_L5 + h * L5_BLOCK, *bias = kernel + (size_t)L4_OUT * L5_OUT;
            for (int k = 0; k < L4_OUT; ++k)
                for (int j = 0; j < L5_OUT; ++j) k5[(size_t)k * L5_ALL + h * L5_OUT + j] = kernel[(size_t)k * L5_OUT + j];
            for (int j = 0; j < L5_OUT; ++j) b5[h * L5_OUT + j] = bias[j];
            const float *hk = weights + off_head_kernel(h), *hb = weights + off_head_bias(h);
            const int width = head_width(h), begin = head_begin(h);
            for (int k = 0; k < L5_OUT; ++k)
                for (int j = 0; j < width; ++j) kh[(size_t)k * PROBS + begin + j] = hk[(size_t)k * width + j];
            for (int j = 0; j < width; ++j) bh[begin + j] = hb[j];
        }
        if (m->put(&m->k3, k3) || m->put(&m->b3, b3) || m->put(&m->k4, k4) || m->put(&m->b4, b4) || m->put(&m->k5, k5) || m->put(&m->b5, b5) ||
            m->put(&m->kh, kh) || m->put(&m->bh, bh))
            return -1;
    }
    // ---- the workspace of a chunk
    const size_t c = (size_t)chunk, ct = (c + TILE - 1) / TILE * TILE;       // (the recurrent kernel writes whole tiles of X)
    if (m->room(&m->G, c * STEPS * 2 * GATES) || m->room(&m->X1, ct * STEPS * BI) || m->room(&m->X2, ct * STEPS * BI) || m->room(&m->L3, c * L3_FLAT) ||
        m->room(&m->L4, c * L4_OUT) || m->room(&m->L5, c * L5_ALL))
        return -1;
    for (hipEvent_t &e : m->ev) MPN_HIP_CHECK(hipEventCreate(&e));
    std::lock_guard<std::mutex> lock(g_clair_mutex);
    *handle = m.get();
    g_clair_models.insert(m.release());
    return 0;
}

extern "C" int32_t mpn_clair_model_free(void *handle) {
    ClairModel *m = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_clair_mutex);
        if (!handle || !g_clair_models.erase(handle)) {
            set_error("mpn_clair_model_free: not a live model");
            return -2;
        }
        m = (ClairModel *)handle;
    }
    (void)hipDeviceSynchronize();
    delete m;
    return 0;
}

extern "C" int64_t mpn_clair_model_chunk(void *handle) {
    ClairModel *m = clair_live(handle);
    if (!m) { set_error("mpn_clair_model_chunk: not a live model"); return -2; }
    return m->chunk;
}

extern "C" int32_t mpn_clair_forward(void *handle, const void *d_tensors, int64_t n, void *d_probs, const mpn_clair_taps *taps) {
    for (double &v : tl_clair_ms) v = 0;
    ClairModel *m = clair_live(handle);
    if (!m || n < 0 || n > 0x7ffffff0 || (n > 0 && (!d_tensors || !d_probs)) || ((uintptr_t)d_tensors & 15)) {
        set_error("mpn_clair_forward: bad arguments (not a live model, no buffers, or tensors that are not 16-byte aligned)");
        return -2;
    }
    if (n == 0) return 0;
    hipStream_t st = 0;
    const int32_t *tensors = (const int32_t *)d_tensors;
    float *probs = (float *)d_probs;
    for (int64_t a = 0; a < n; a += m->chunk) {
        const int64_t nc = std::min(m->chunk, n - a);
        const unsigned tiles = (unsigned)((nc + TILE - 1) / TILE);
        MPN_HIP_CHECK(hipEventRecord(m->ev[0], st));
        if (clair_gemm<int32_t, false>(st, tensors + a * CELLS, nc * STEPS, FEATURES, m->wx[0], 2 * GATES, m->bx[0], m->G)) return -1;
        MPN_HIP_CHECK(hipEventRecord(m->ev[1], st));
        hipLaunchKernelGGL(clair_rec_kernel, dim3(tiles, 2), dim3(REC_THREADS), 0, st, (const float *)m->G, (const float *)m->image[0], m->X1, nc);
        MPN_HIP_CHECK(hipGetLastError());
        MPN_HIP_CHECK(hipEventRecord(m->ev[2], st));
        if (clair_gemm<float, false>(st, m->X1, nc * STEPS, BI, m->wx[1], 2 * GATES, m->bx[1], m->G)) return -1;
        MPN_HIP_CHECK(hipEventRecord(m->ev[3], st));
        hipLaunchKernelGGL(clair_rec_kernel, dim3(tiles, 2), dim3(REC_THREADS), 0, st, (const float *)m->G, (const float *)m->image[1], m->X2, nc);
        MPN_HIP_CHECK(hipGetLastError());
        MPN_HIP_CHECK(hipEventRecord(m->ev[4], st));
        hipLaunchKernelGGL(clair_l3_kernel, dim3((unsigned)((nc + L3_ROWS - 1) / L3_ROWS)), dim3(BI), 0, st, (const float *)m->X2, (const float *)m->k3,
                           (const float *)m->b3, m->L3, nc);
        MPN_HIP_CHECK(hipGetLastError());
        MPN_HIP_CHECK(hipEventRecord(m->ev[5], st));
        if (clair_gemm<float, true>(st, m->L3, nc, L3_FLAT, m->k4, L4_OUT, m->b4, m->L4)) return -1;
        MPN_HIP_CHECK(hipEventRecord(m->ev[6], st));
        if (clair_gemm<float, true>(st, m->L4, nc, L4_OUT, m->k5, L5_ALL, m->b5, m->L5)) return -1;
        hipLaunchKernelGGL(clair_heads_kernel, dim3((unsigned)((nc + HEAD_ROWS - 1) / HEAD_ROWS)), dim3(HEAD_THREADS), 0, st, (const float *)m->L5,
                           (const float *)m->kh, (const float *)m->bh, probs + a * PROBS, nc);
        MPN_HIP_CHECK(hipGetLastError());
        MPN_HIP_CHECK(hipEventRecord(m->ev[7], st));
        if (taps) {
            const size_t f = sizeof(float);
            if (taps->lstm1) MPN_HIP_CHECK(hipMemcpyAsync((float *)taps->lstm1 + a * STEPS * BI, m->X1, (size_t)nc * STEPS * BI * f, hipMemcpyDeviceToDevice, st));
            if (taps->lstm2) MPN_HIP_CHECK(hipMemcpyAsync((float *)taps->lstm2 + a * STEPS * BI, m->X2, (size_t)nc * STEPS * BI * f, hipMemcpyDeviceToDevice, st));
            if (taps->l3) MPN_HIP_CHECK(hipMemcpyAsync((float *)taps->l3 + a * L3_FLAT, m->L3, (size_t)nc * L3_FLAT * f, hipMemcpyDeviceToDevice, st));
            if (taps->l4) MPN_HIP_CHECK(hipMemcpyAsync((float *)taps->l4 + a * L4_OUT, m->L4, (size_t)nc * L4_OUT * f, hipMemcpyDeviceToDevice, st));
        }
        MPN_HIP_CHECK(hipEventRecord(m->ev[8], st));
        MPN_HIP_CHECK(hipStreamSynchronize(st));
        float ms[8];
        for (int i = 0; i < 8; ++i) MPN_HIP_CHECK(hipEventElapsedTime(&ms[i], m->ev[i], m->ev[i + 1]));
        tl_clair_ms[0] += ms[0] + ms[2];
        tl_clair_ms[1] += ms[1] + ms[3];
        tl_clair_ms[2] += ms[4];
        tl_clair_ms[3] += ms[5];
        tl_clair_ms[4] += ms[6];
        for (int i = 0; i < 8; ++i) tl_clair_ms[5] += ms[i];
    }
    return 0;
}
