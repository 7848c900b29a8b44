// The resident core of mpn_bgzf_compress (csrc/bgzf_kernels.hip): payloads that already lie on the device -> packed BGZF blocks on
// the device.  mpn_bgzf_compress uploads, calls the two steps and downloads; the device BAM writer (csrc/bam_out_kernels.hip)
// calls them on the payloads its gather wrote.  A block's bytes depend on its payload and the mode alone.
#pragma once
#include "mpn_common.h"

namespace mpn {

struct BgzfWork {
    DevBuf<uint8_t> slots, out;       // out: the packed blocks after bgzf_pack_resident
    DevBuf<int64_t> oo;
    DevBuf<uint32_t> tok;
    DevBuf<int32_t> sizes;
    DevBuf<int> flag;
};

// d_pay: the payload bytes, starting with block 0's (pay_bytes of them); d_po: n_blocks + 1 resident offsets (only their differences
// and d_po[0] as the origin are used); every block has 0..65280 bytes (the caller has checked).  Deflates into slots, scans the
// sizes, downloads out_off (n_blocks + 1 host entries) and waits.  -> the bytes of all blocks, or -1.  tl_bgzf_ms[0] is set.
int64_t bgzf_deflate_resident(const uint8_t *d_pay, int64_t pay_bytes, const int64_t *d_po, int64_t n_blocks, int32_t mode, hipStream_t st,
                              BgzfWork &w, int64_t *out_off);
// slots -> w.out (total bytes), queued on st between tm's two events; the caller synchronises before it reads either
int bgzf_pack_resident(const int64_t *d_po, int64_t n_blocks, int64_t total, hipStream_t st, BgzfWork &w, DevTimer &tm);

}  // namespace mpn
