/*
 * mpn_clair.h -- C-ABI of Clair's network on the GPU (csrc/clair_net_kernels.hip): the probabilities that `call_var
 * --output_for_ensemble` computes with one model (clair/model.py, structure 2BiLSTM, inference only), for the tensors that
 * mpn_tensor_fill left in HBM (megapath_nano_amd/clair_net.py; the rules are DESIGN.md section 6 item 18).
 *
 *   mpn_clair_model_create   the variables, in the one flat host layout below -> a handle: the variables on the device in the
 *                            layouts of the kernels, and the workspace of one chunk
 *   mpn_clair_forward        n tensors (DEVICE, int32) -> n x 90 float32 (DEVICE); nothing crosses PCIe
 *   mpn_clair_model_free
 *
 * All matrix products are float32 on the f32-input MFMA, a k-ordered fmaf chain: the output of a tensor does not depend on the
 * tensors around it, on n, or on the chunk, and is the same from run to run.  The arithmetic shared with the host is
 * csrc/clair_net_core.h (scripts/clair_net_host_check.cpp runs it serially).  Calling rules as in mpn_tensor.h: a call returns
 * when its results are in place, the default stream is used, 0 = done, -1 = device error (mpn_last_error()), -2 = bad arguments.
 *
 * The flat layout (MPN_CLAIR_WEIGHTS float32; every kernel row-major as TensorFlow keeps it, [inputs][outputs]):
 *   for LSTM1 (inputs 32), LSTM2 (inputs 256); for fw, bw:   kernel [inputs + 128][512]   rows x then h; columns i, j, f, o
 *                                                            bias   [512]
 *   L3/Unit_0 .. Unit_255   kernel [33][30] each, then bias [30] each
 *   L4                      kernel [7680][192], bias [192]
 *   L5_1 .. L5_4            kernel [192][96], bias [96], each
 *   Prediction/Y_base_change_logits [96][21], bias; Y_genotype_logits [96][3], bias; Y_indel_length_logits_1 [96][33], bias;
 *   Y_indel_length_logits_2 [96][33], bias
 */
#ifndef MPN_CLAIR_H
#define MPN_CLAIR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_CLAIR_TILE 32               /* batch rows one workgroup of the recurrent kernel carries */
#define MPN_CLAIR_STEPS 33
#define MPN_CLAIR_FEATURES 32
#define MPN_CLAIR_UNITS 128
#define MPN_CLAIR_PROBS 90              /* 21 | 3 | 33 | 33 */
#define MPN_CLAIR_WEIGHTS 2377818
#define MPN_CLAIR_CHUNK_DEFAULT 4096    /* MPN_CLAIR_CHUNK: tensors of one pass; about 236 KiB of workspace each, 0.93 GiB */
#define MPN_CLAIR_CHUNK_MAX 65536

/* Device buffers that receive the layer outputs of all n tensors; any may be NULL. */
typedef struct {
    void *lstm1;    /* n x 33 x 256: [tensor][step][fw 128 | bw 128] */
    void *lstm2;    /* n x 33 x 256 */
    void *l3;       /* n x 7680: index u * 256 + c */
    void *l4;       /* n x 192 */
} mpn_clair_taps;

/* weights (host): count = MPN_CLAIR_WEIGHTS floats in the layout above; -2 otherwise.  The environment's MPN_CLAIR_CHUNK (1 ..
 * MPN_CLAIR_CHUNK_MAX; default MPN_CLAIR_CHUNK_DEFAULT) is read here. */
int32_t mpn_clair_model_create(const float *weights, int64_t count, void **handle);
/* -2 for a handle that is not a live model */
int32_t mpn_clair_model_free(void *handle);
/* the chunk of a live model, -2 otherwise */
int64_t mpn_clair_model_chunk(void *handle);

/* d_tensors (DEVICE): n x 1056 int32, cell ((index * 8 + row) * 4 + channel) as mpn_tensor_fill writes them.  d_probs (DEVICE):
 * n x 90 float32.  Rows from n on are neither read nor written.  taps may be NULL. */
int32_t mpn_clair_forward(void *handle, const void *d_tensors, int64_t n, void *d_probs, const mpn_clair_taps *taps);

/* Device time of the calling thread's last forward, summed over its chunks, in milliseconds: the two input projections, the two
 * recurrent passes, L3, L4, L5 with the heads and softmaxes, and the whole call (tap copies included).  Any pointer may be NULL. */
void mpn_clair_last_device_ms(double *project_ms, double *recurrent_ms, double *l3_ms, double *l4_ms, double *heads_ms, double *total_ms);

/* MPN_CLAIR_TILE */
int32_t mpn_clair_tile(void);

#ifdef __cplusplus
}
#endif
#endif
