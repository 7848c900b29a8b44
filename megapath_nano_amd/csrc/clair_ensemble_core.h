// The arithmetic and the index checks of the averaging of Clair's lines per site (include/mpn_ensemble.h), shared by the kernel
// (csrc/clair_ensemble_kernels.hip) and the serial host build (scripts/clair_ensemble_host_check.cpp).  Semantics:
// clair/post_processing/ensemble.py.
//
// Every double operation whose rounding is part of the contract is spelled through ens_mul / ens_add / ens_div / ens_fma, whose
// bodies switch contraction off: hipcc contracts `a * b - c` into one fma by default (and HIP's __dmul_rn is a plain `*` that it
// contracts as well), while ens_round_micro relies on the PRODUCT being rounded before its residual is taken.  g++ has no such
// pragma: a host build is compiled with -ffp-contract=off (x86-64 without -mfma cannot contract; other targets can).
#ifndef MPN_CLAIR_ENSEMBLE_CORE_H
#define MPN_CLAIR_ENSEMBLE_CORE_H
#include <stdint.h>
#include "../../include/mpn_ensemble.h"

#if defined(__HIPCC__)
#define ENS_HD __host__ __device__ inline
#else
#define ENS_HD inline
#endif

#if defined(__clang__)
#define ENS_NO_CONTRACT _Pragma("clang fp contract(off)")
#define ENS_UNROLLED _Pragma("unroll")
#else
#define ENS_NO_CONTRACT
#define ENS_UNROLLED _Pragma("GCC unroll 8")
#endif

namespace mpn_ens {

constexpr int CELLS = MPN_ENS_CELLS, PROBS = MPN_ENS_PROBS, COLS = MPN_ENS_CELLS + MPN_ENS_PROBS;
constexpr int CHUNK = 64;                                   // columns of a work item: a wave, a lane per column
constexpr int CHUNKS = (COLS + CHUNK - 1) / CHUNK;          // 18 items per site

ENS_HD double ens_mul(double a, double b) {
    ENS_NO_CONTRACT
    return a * b;
}
ENS_HD double ens_add(double a, double b) {
    ENS_NO_CONTRACT
    return a + b;
}
ENS_HD double ens_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
ENS_HD double ens_fma(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fma_rn(a, b, c);
#else
    return __builtin_fma(a, b, c);
#endif
}
ENS_HD double ens_floor(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return floor(a);
#else
    return __builtin_floor(a);
#endif
}
ENS_HD double ens_rint(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return rint(a);
#else
    return __builtin_rint(a);
#endif
}

// The float64 a line adds.  float32 (the network's output): what float('%.6f' % p) gives; (double)p * 1e6 is exact (24 bits times
// 15625 * 2^6, see call_quantize in clair_call_core.h), so rint rounds what %.6f rounds.  float64 (parsed text): as it is.
ENS_HD double ens_addend(float p) { return ens_div(ens_rint(ens_mul((double)p, 1.0e6)), 1.0e6); }
ENS_HD double ens_addend(double p) { return p; }

// Inside the domain of ens_round_micro: finite and |q| < 2^31 (2^31 * 1e6 < 2^51: every integer there is a float64).
ENS_HD bool ens_in_domain(double q) { return q > -2147483648.0 && q < 2147483648.0; }

// The integer n of '%.6f' % a for 0 <= a < 2^31, n / 10^6 being the decimal printed: the EXACT binary value of a, times 10^6,
// rounded to the nearest integer with ties to even (glibc's printf and CPython's format round the exact value).
// rint(a * 1e6) is not that: the product is rounded first, and may land on a tie that the exact value only comes near (an odd sum
// of micro-units halved), or leave one.  So: p = fl(a * 1e6) and its exact residual r = a * 1e6 - p (one fma: the residual of a
// product is a float64).  With f = floor(p): e = (p - f) - 0.5 is exact (p, f and 0.5 are multiples of ulp(p), or p < 1 and only
// the sign of e matters), and if e != 0 then |e| >= ulp(p) > |r|, so the sign of e decides; if e == 0 the sign of r decides; if
// both are 0 the value is an exact tie (a is an odd multiple of 1/128 then) and the even neighbour is taken.
ENS_HD int64_t ens_round_micro(double a) {
    const double p = ens_mul(a, 1.0e6);
    const double r = ens_fma(a, 1.0e6, -p);
    const double f = ens_floor(p);
    const double e = ens_add(ens_add(p, -f), -0.5);
    const int64_t n = (int64_t)f;
    const bool up = e > 0.0 || (e == 0.0 && (r > 0.0 || (r == 0.0 && (n & 1))));
    return n + (up ? 1 : 0);
}

// What `{:.6f}` and read_probability_lines' parse (float64, then float32) leave of q = sum / count; *micro (may be NULL) = the
// integer printed, with the sign of q (0 for a negative zero: the float32 keeps that sign).  Outside the domain: (float)q, 0.
ENS_HD float ens_result(double q, int64_t *micro) {
    if (!ens_in_domain(q)) {
        if (micro) *micro = 0;
        return (float)q;
    }
    const bool neg = q < 0.0 || (q == 0.0 && ens_div(1.0, q) < 0.0);
    const int64_t n = ens_round_micro(neg ? -q : q);
    if (micro) *micro = neg ? -n : n;
    const double v = ens_div((double)n, 1.0e6);               // correctly rounded, as the parse of the decimal is
    return (float)(neg ? -v : v);
}

constexpr int UNROLL = 8;      // lines whose loads are in flight together: a 400-line site is 50 round trips to memory, not 400

// One column of one site: the lines rows[b .. e) in their order, UNROLL of them loaded before they are added.  Cells: the int64
// sum (the caller tests it against int32).
ENS_HD int64_t ens_cell(const int32_t *__restrict__ tensors, const int32_t *__restrict__ rows, int64_t b, int64_t e, int col) {
    const int32_t *__restrict__ from = tensors + col;
    int64_t sum = 0, i = b;
    for (; i + UNROLL <= e; i += UNROLL) {
        int32_t v[UNROLL];
        ENS_UNROLLED
        for (int k = 0; k < UNROLL; ++k) v[k] = from[(int64_t)rows[i + k] * CELLS];
        ENS_UNROLLED
        for (int k = 0; k < UNROLL; ++k) sum += v[k];
    }
    for (; i < e; ++i) sum += from[(int64_t)rows[i] * CELLS];
    return sum;
}

// Probabilities: the first line's addend, then one float64 addition per further line, in order; divided by the count.
template <typename P>
ENS_HD double ens_mean(const P *__restrict__ probs, const int32_t *__restrict__ rows, int64_t b, int64_t e, int col) {
    const P *__restrict__ from = probs + col;
    double sum = ens_addend(from[(int64_t)rows[b] * PROBS]);
    int64_t i = b + 1;
    for (; i + UNROLL <= e; i += UNROLL) {
        P v[UNROLL];
        ENS_UNROLLED
        for (int k = 0; k < UNROLL; ++k) v[k] = from[(int64_t)rows[i + k] * PROBS];
        ENS_UNROLLED
        for (int k = 0; k < UNROLL; ++k) sum = ens_add(sum, ens_addend(v[k]));
    }
    for (; i < e; ++i) sum = ens_add(sum, ens_addend(from[(int64_t)rows[i] * PROBS]));
    return ens_div(sum, (double)(e - b));
}

// The checks of the lines and the CSR, and the gather of the row indices into the order of the CSR: row_t[i] / row_p[i] (room for
// site_off[n_sites] each) = the tensor / probability row of entry i.  used: room for n_out bytes.  0, or the MPN_ENS_BAD_* of the
// first thing that is wrong, with *at = the line, entry, site or slot.
inline int ens_check_gather(int64_t n_lines, const int32_t *tensor_row, const int32_t *prob_row, int64_t n_t, int64_t n_p, int64_t n_sites,
                            const int64_t *site_off, const int32_t *site_lines, const int32_t *out_slot, int64_t n_out, int32_t *row_t, int32_t *row_p,
                            uint8_t *used, int64_t *at) {
    for (int64_t i = 0; i < n_lines; ++i)
        if (tensor_row[i] < 0 || tensor_row[i] >= n_t || prob_row[i] < 0 || prob_row[i] >= n_p) { *at = i; return MPN_ENS_BAD_ROW; }
    if (n_sites > 0 && site_off[0] != 0) { *at = 0; return MPN_ENS_BAD_SITE; }
    for (int64_t s = 0; s < n_sites; ++s)
        if (site_off[s + 1] <= site_off[s] || site_off[s + 1] > 0x7ffffff0) { *at = s; return MPN_ENS_BAD_SITE; }      // a site without lines
    const int64_t n_entries = n_sites > 0 ? site_off[n_sites] : 0;
    for (int64_t i = 0; i < n_entries; ++i) {
        const int32_t line = site_lines[i];
        if (line < 0 || line >= n_lines) { *at = i; return MPN_ENS_BAD_ENTRY; }
        row_t[i] = tensor_row[line];
        row_p[i] = prob_row[line];
    }
    for (int64_t k = 0; k < n_out; ++k) used[k] = 0;
    int64_t n_used = 0;
    for (int64_t s = 0; s < n_sites; ++s) {
        const int32_t slot = out_slot[s];
        if (slot == -1) continue;
        if (slot < 0 || slot >= n_out || used[slot]) { *at = s; return MPN_ENS_BAD_SLOT; }                              // outside, or used twice
        used[slot] = 1;
        ++n_used;
    }
    if (n_used != n_out) { *at = n_used; return MPN_ENS_BAD_SLOT; }                                                    // a slot nobody writes
    return 0;
}

}  // namespace mpn_ens
#endif
