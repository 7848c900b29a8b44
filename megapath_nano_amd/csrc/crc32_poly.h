// CRC-32 (RFC 1952 section 8) as polynomial arithmetic mod P, for the kernels that take the CRC of a byte string in parallel:
// bgzf_deflate_kernel stage E (csrc/bgzf_kernels.hip) and the wave flush of gzip_inflate_kernel (csrc/inflate_kernels.hip).
// It compiles for the device and for the host with plain g++ (scripts/crc32_host_check.cpp, scripts/inflate_host_check.cpp).
//
// Registers are reflected: bit 31 is x^0.  The register after a byte string is linear in (register before, bytes), so a string
// cut into slices can be summed: every slice's CRC from a ZERO register, times x^(8 * bytes behind the slice), xor over the
// slices (crc_slice), plus the old register times x^(8 * bytes in all) (crc_join).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CRC_HD __host__ __device__ __forceinline__
#else
#define CRC_HD inline
#endif

namespace mpn_crc {

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr int CRC_XPOW8_BITS = 17;       // crc_xpow8(k) is valid for k < 2^17

// entry c (0..255) of the byte table: a register with c in its low byte, after eight steps
CRC_HD uint32_t crc_entry(uint32_t c) {
    for (int k = 0; k < 8; ++k) c = (c & 1) ? CRC_POLY ^ (c >> 1) : c >> 1;
    return c;
}
// product of two polynomials mod P
CRC_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) r ^= b;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return r;
}
// x^(8k) mod P by squaring, for 0 <= k < 2^CRC_XPOW8_BITS: a BGZF payload has at most 65 280 bytes, an inflate flush fewer than
// 2^15.  (The loop leaves when k is used up; the bound is what lets the compiler unroll it.)
CRC_HD uint32_t crc_xpow8(uint32_t k) {
    uint32_t r = 0x80000000u, b = 0x00800000u;
    for (int i = 0; i < CRC_XPOW8_BITS && k; ++i, k >>= 1) {
        if (k & 1) r = crc_mul(r, b);
        b = crc_mul(b, b);
    }
    return r;
}
// what a slice adds to the register: c = the slice's CRC from a zero register, behind = the bytes of the string after the slice
CRC_HD uint32_t crc_slice(uint32_t c, uint32_t behind) { return crc_mul(c, crc_xpow8(behind)); }
// the register after len more bytes: old = the register before them, slices = the xor of their crc_slice values
CRC_HD uint32_t crc_join(uint32_t old, uint32_t len, uint32_t slices) { return crc_mul(old, crc_xpow8(len)) ^ slices; }

}  // namespace mpn_crc
