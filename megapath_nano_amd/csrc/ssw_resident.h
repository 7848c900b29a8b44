// The core of the batched SSW (csrc/ssw_kernels.hip) on reads and references that are already in HBM, and whose results stay
// there: what mpn_ssw_align_batch runs after its upload, and what csrc/local_realign_kernels.hip runs on the fragments it has just
// written.  Internal to libmpn.so.
#pragma once
#include "mpn_common.h"

namespace mpn {

// Everything a call leaves behind; the device buffers live as long as the struct.
//   res      9 rows of n_pairs int32: score1, score2, ref_begin1, ref_end1, read_begin1, read_end1, ref_end2, status (the final
//            one, as status_h), need_cigar
//   cig      the CIGARs: pair i's operations are cig[cig_end[i] - cig_len[i] .. cig_end[i]) (cig_len 0: none)
// and the host's copies of the small ones (the band rounds are planned on the host).
struct SswResident {
    DevBuf<int64_t> read_off, ref_off, mcol_off, cig_end;
    DevBuf<int32_t> read_len, ref_len, mask, res, order, cig_len;
    DevBuf<uint16_t> mcol;
    DevBuf<uint32_t> cig;
    std::vector<int32_t> res_h, status_h, cig_len_h;
    std::vector<char> launched;          // 0: refused before the launch (status_h says why); its result row is zero
    std::vector<int64_t> cig_end_h;
    int64_t cig_total = 0;
};

// d_reads, d_refs: DEVICE.  Everything else as mpn_ssw_align_batch takes it (host).  Workspace on the device, per pair: 36 bytes
// of results, 2 bytes per reference column (rounded up to 64 columns), 4 bytes per CIGAR slot (reference span + read span + 4),
// and per band round (2 * band + 1) * read span bytes of direction codes (at most 2 GiB a launch).
int ssw_resident(int32_t n_pairs, const int8_t *d_reads, const int64_t *read_off, const int32_t *read_len, const int8_t *d_refs,
                 const int64_t *ref_off, const int32_t *ref_len, const int8_t *mat, int32_t n, int8_t score_size, uint8_t gap_open,
                 uint8_t gap_extend, uint8_t flag, uint16_t filters, int32_t filterd, const int32_t *mask_len, SswResident &R);

}  // namespace mpn
