// Clair's lines averaged per site, behind include/mpn_ensemble.h.  Semantics: clair/post_processing/ensemble.py (DESIGN.md section 6
// item 21); the arithmetic and the checks shared with the host are csrc/clair_ensemble_core.h.
//
//   ens_kernel<P>   a wave per (site, 64 columns) and a lane per column, so that a wave-instruction reads 256 consecutive bytes of a
//                   row and a deep site is spread over 18 waves instead of holding one.  A wave is sequential over the site's
//                   lines (the order of the float64 additions is the contract) but loads UNROLL of them before it adds (ens_cell,
//                   ens_mean: the loops the host build runs), so that a 400-line site is 50 round trips to memory, not 400.  The row
//                   indices are wave-uniform.  Columns 0 .. 1055 are int64 sums of int32 cells, columns 1056 .. 1145 float64 means
//                   (P: float or double), rounded by ens_result.
//                   Plain vector stores; the one atomic is the minimum over the sites whose sum leaves int32.  No LDS.
#include "mpn_common.h"
#include "clair_ensemble_core.h"

namespace mpn {

using namespace mpn_ens;

static thread_local double tl_ens_ms = 0;

constexpr int ENS_WAVES = 4;       // waves of a block: 256 threads

template <typename P>
__global__ __launch_bounds__(ENS_WAVES * 64) void ens_kernel(const int32_t *__restrict__ tensors, const P *__restrict__ probs, const int32_t *__restrict__ row_t,
                                                             const int32_t *__restrict__ row_p, const int64_t *__restrict__ site_off,
                                                             const int32_t *__restrict__ out_slot, int64_t n_sites, int32_t *__restrict__ out_t,
                                                             float *__restrict__ out_p, int64_t *__restrict__ out_micro, int32_t *__restrict__ bad_site) {
    const int64_t item = (int64_t)blockIdx.x * ENS_WAVES + (threadIdx.x >> 6);
    if (item >= n_sites * CHUNKS) return;
    const int64_t site = item / CHUNKS;
    const int col = (int)(item % CHUNKS) * CHUNK + (int)(threadIdx.x & 63);
    const int64_t slot = out_slot[site];
    if (slot < 0 || col >= COLS) return;
    const int64_t b = site_off[site], e = site_off[site + 1];
    if (col < CELLS) {
        const int64_t sum = ens_cell(tensors, row_t, b, e, col);
        if (sum != (int64_t)(int32_t)sum) atomicMin(bad_site, (int32_t)site);
        out_t[slot * CELLS + col] = (int32_t)sum;
    } else {
        const int pc = col - CELLS;
        int64_t micro = 0;
        out_p[slot * PROBS + pc] = ens_result(ens_mean(probs, row_p, b, e, pc), &micro);
        if (out_micro) out_micro[slot * PROBS + pc] = micro;
    }
}

}  // namespace mpn

using namespace mpn;

extern "C" void mpn_clair_ensemble_last_device_ms(double *ms) {
    if (ms) *ms = tl_ens_ms;
}

extern "C" int32_t mpn_clair_ensemble(int64_t n_lines, const int32_t *tensor_row, const int32_t *prob_row, const void *d_tensors, int64_t n_t,
                                      const void *d_probs, int64_t n_p, int32_t probs_f64, int64_t n_sites, const int64_t *site_off,
                                      const int32_t *site_lines, const int32_t *out_slot, int64_t n_out, void *d_out_tensors, void *d_out_probs,
                                      void *d_out_micro, int64_t *bad_site) {
    tl_ens_ms = 0;
    const int64_t most = 0x7ffffff0 / (MPN_ENS_CELLS / 16);      // rows of a block, lines and sites: every index and item number stays far inside int64
    if (n_lines < 0 || n_lines > most || n_t < 0 || n_t > most || n_p < 0 || n_p > most || n_sites < 0 || n_sites > most || n_out < 0 || n_out > n_sites ||
        !bad_site || (n_lines > 0 && (!tensor_row || !prob_row)) || (n_sites > 0 && (!site_off || !site_lines || !out_slot || n_lines == 0)) ||
        (n_t > 0 && !d_tensors) || (n_p > 0 && !d_probs) || (n_out > 0 && (!d_out_tensors || !d_out_probs))) {
        set_error("mpn_clair_ensemble: bad arguments");
        return -2;
    }
    *bad_site = -1;
    if (n_sites == 0) return 0;
    if (site_off[n_sites] < 0 || site_off[n_sites] > most) {
        set_error("mpn_clair_ensemble: the offsets of the sites end at %lld", (long long)site_off[n_sites]);
        return -2;
    }
    for (int64_t s = 0; s < n_sites; ++s)            // (ens_check_gather reads site_off[n_sites] entries: the offsets must not pass it)
        if (site_off[s] < 0 || site_off[s] > site_off[n_sites]) {
            set_error("mpn_clair_ensemble: site %lld: its offset lies outside the entries", (long long)s);
            return -2;
        }
    const size_t n_entries = (size_t)site_off[n_sites];
    int32_t *rows = (int32_t *)malloc((2 * n_entries + 1) * sizeof(int32_t));
    uint8_t *used = (uint8_t *)malloc((size_t)n_out + 1);
    int64_t at = -1;
    const int what = rows && used ? ens_check_gather(n_lines, tensor_row, prob_row, n_t, n_p, n_sites, site_off, site_lines, out_slot, n_out, rows,
                                                     rows + n_entries, used, &at)
                                  : -1;
    free(used);
    if (what != 0) {
        free(rows);
        static const char *const why[] = {"", "line: its tensor or probability row lies outside the block", "site: no lines, or offsets that do not ascend from 0",
                                          "entry of the sites' lists: not a line",
                                          "site: its output slot lies outside the output or is used twice (or the number of used slots: a slot is not used)"};
        if (what < 0) set_error("mpn_clair_ensemble: out of host memory");
        else set_error("mpn_clair_ensemble: %lld, a %s", (long long)at, why[what]);
        return what < 0 ? -1 : -2;
    }
    if (n_out == 0) {
        free(rows);
        return 0;
    }
    hipStream_t st = 0;
    DevBuf<int32_t> d_rows, d_slot, d_bad;
    DevBuf<int64_t> d_off;
    DevTimer tm;
    const int32_t none = 0x7fffffff;
    const int up = d_rows.upload(rows, 2 * n_entries, st) || d_off.upload(site_off, (size_t)n_sites + 1, st) || d_slot.upload(out_slot, (size_t)n_sites, st) ||
                   d_bad.upload(&none, 1, st);
    const hipError_t copied = hipStreamSynchronize(st);
    free(rows);                                         // (the copies above have ended)
    if (up) return -1;
    if (copied != hipSuccess) {
        set_error("mpn_clair_ensemble: the upload of the lists failed: %s", hipGetErrorString(copied));
        return -1;
    }
    if (tm.start(st)) return -1;
    const int64_t items = n_sites * CHUNKS;
    const dim3 grid((unsigned)((items + ENS_WAVES - 1) / ENS_WAVES)), block(ENS_WAVES * 64);
    const int32_t *rt = d_rows.p, *rp = d_rows.p + n_entries;
    if (probs_f64)
        hipLaunchKernelGGL(ens_kernel<double>, grid, block, 0, st, (const int32_t *)d_tensors, (const double *)d_probs, rt, rp, (const int64_t *)d_off.p,
                           (const int32_t *)d_slot.p, n_sites, (int32_t *)d_out_tensors, (float *)d_out_probs, (int64_t *)d_out_micro, d_bad.p);
    else
        hipLaunchKernelGGL(ens_kernel<float>, grid, block, 0, st, (const int32_t *)d_tensors, (const float *)d_probs, rt, rp, (const int64_t *)d_off.p,
                           (const int32_t *)d_slot.p, n_sites, (int32_t *)d_out_tensors, (float *)d_out_probs, (int64_t *)d_out_micro, d_bad.p);
    MPN_HIP_CHECK(hipGetLastError());
    int32_t bad = none;
    if (tm.stop(st) || d_bad.download(&bad, 1, st)) return -1;
    MPN_HIP_CHECK(hipStreamSynchronize(st));
    if (tm.elapsed_ms(&tl_ens_ms)) return -1;
    if (bad != none) *bad_site = bad;
    return 0;
}
