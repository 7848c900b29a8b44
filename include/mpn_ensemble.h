/*
 * mpn_ensemble.h -- C-ABI of the averaging of Clair's lines per site on the GPU (csrc/clair_ensemble_kernels.hip), the drop-in for
 * clair/post_processing/ensemble.py, which `clair.py ensemble` runs between the models and call_var --input_probabilities
 * (megapath_nano_amd/clair_ensemble.py; the rules are DESIGN.md section 6 item 21).
 *
 *   mpn_clair_ensemble   L lines over resident tensors and probabilities, grouped by the host -> one line per site that is kept
 *
 * The arithmetic shared by host and device is csrc/clair_ensemble_core.h (scripts/clair_ensemble_host_check.cpp runs it serially).
 * Calling rules as in mpn_call.h: the call returns when its results are in place, the default stream is used, 0 = done, -1 = device
 * error (mpn_last_error()), -2 = bad arguments (mpn_last_error() names the first line, entry, site or slot that is wrong).
 */
#ifndef MPN_ENSEMBLE_H
#define MPN_ENSEMBLE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_ENS_CELLS 1056           /* int32 of a tensor: 33 x 8 x 4 */
#define MPN_ENS_PROBS 90             /* gt21 (21) | genotype (3) | length_1 (33) | length_2 (33) */

/* what ens_check_gather (csrc/clair_ensemble_core.h) finds */
#define MPN_ENS_BAD_ROW 1            /* a line's tensor or probability row lies outside its block */
#define MPN_ENS_BAD_SITE 2           /* the offsets do not start at 0, or a site has no lines */
#define MPN_ENS_BAD_ENTRY 3          /* an entry of the CSR is not a line */
#define MPN_ENS_BAD_SLOT 4           /* an output slot outside 0 .. n_out - 1, used twice, or not used at all */

/* Line i (host arrays of n_lines) is the pair (tensor_row[i], prob_row[i]) of row indices into d_tensors (DEVICE, int32, n_t rows of
 * 1056) and d_probs (DEVICE, n_p rows of 90; float32, or float64 with probs_f64 != 0), so that K models over one tensor block need
 * no K copies of it; a tensor is still summed once per line that names it.  The grouping is the host's: site s (in the order of
 * first appearance) has the lines site_lines[site_off[s] .. site_off[s + 1]) (host; at least one, in input order) and is written to
 * row out_slot[s] (host; -1: below the minimum count, not written) of d_out_tensors (DEVICE, int32, n_out rows of 1056) and
 * d_out_probs (DEVICE, float32, n_out rows of 90); every slot 0 .. n_out - 1 is used once.
 *   cells          the sum over the site's lines in int64.  *bad_site = -1, or the smallest site with a sum outside int32: the
 *                  results are not to be used then.
 *   probabilities  the addends in float64 (float32 input: float('%.6f' % p); float64 input: as it is), added in the order of the
 *                  lines, divided by their number, printed `{:.6f}` (the exact binary value rounded, ties to even) and parsed through
 *                  float64 to float32.  d_out_micro (DEVICE, int64, n_out rows of 90; may be NULL): the integer of that print in
 *                  units of 10^-6, signed (a value of 8 or more has no float32 that prints back to its own text).
 * A wave per site and 64 columns, a lane per column, sequential over the site's lines; plain vector stores.  The results are the
 * same from run to run. */
int32_t mpn_clair_ensemble(int64_t n_lines, const int32_t *tensor_row, const int32_t *prob_row, const void *d_tensors, int64_t n_t,
                           const void *d_probs, int64_t n_p, int32_t probs_f64, int64_t n_sites, const int64_t *site_off, const int32_t *site_lines,
                           const int32_t *out_slot, int64_t n_out, void *d_out_tensors, void *d_out_probs, void *d_out_micro, int64_t *bad_site);

/* Device time of the calling thread's last mpn_clair_ensemble, in milliseconds. */
void mpn_clair_ensemble_last_device_ms(double *ms);

#ifdef __cplusplus
}
#endif
#endif
