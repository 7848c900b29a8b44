// The host half of the stage-test entries' input layer: what mpn_ext_dp_batch, mpn_aln_tags_batch, mpn_aln_finish_batch (pairs
// of code strings, optionally with an aligned interval and a CIGAR), the CSR entries (mpn_chain_batch, mpn_hit_select_batch,
// mpn_ext_plan_batch, mpn_stitch_batch) and mpn_seed_anchors_batch (a made index, made minimizers, options and knobs) check and lay
// out before anything is uploaded.  Plain C++ without HIP or the library, so that scripts/stage_input_host_check.cpp runs it under
// the host's sanitizers (tests/test_stage_input.py).
// Every function takes the entry's name and reports through the caller's sink: set_error in the library.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace mpn_stage {

typedef void (*err_fn)(const char *fmt, ...);

// rows of a CSR array and the totals of a pair set: what the entries' 32-bit counts and the host buffers sized from them hold
constexpr int64_t STAGE_MAX = 0x3fffffff;

// CSR offsets off[0 .. n]: start at 0, never decrease, no row above STAGE_MAX
inline bool stage_csr_ok(const char *who, int32_t n, const int64_t *off, err_fn err) {
    if (n <= 0) return true;
    if (off[0] != 0) { err("%s: offsets do not start at 0", who); return false; }
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > STAGE_MAX) { err("%s: read %d: offsets out of order", who, i); return false; }
    return true;
}

// ---- mpn_seed_anchors_batch: a made index, made minimizers, options and knobs -------------------------------------------------
// The index of the caller: n_seq targets of lens bases, n_keys keys (strictly ascending, inside 2k bits) with their positions by
// key_off, every position word rid << 32 | position << 1 | strand inside its target.  What the lookup, the filter, the emission and
// the sort's bin index with.
inline bool stage_seed_index_ok(const char *who, int32_t k, int32_t n_seq, const int32_t *lens, int64_t n_keys, const uint64_t *keys,
                                const int64_t *key_off, const uint64_t *pos, err_fn err) {
    if (k < 1 || k > 28 || n_seq < 1 || n_keys < 0 || n_keys > STAGE_MAX || !lens || !key_off || (n_keys > 0 && !keys)) {
        err("%s: index: k outside 1 .. 28, no target, a key count outside 0 .. 2^30 - 1 or an array missing", who); return false;
    }
    for (int32_t i = 0; i < n_seq; ++i)
        if (lens[i] < 0) { err("%s: index: target %d: negative length", who, i); return false; }
    if (n_keys == 0) {
        if (key_off[0] != 0) { err("%s: offsets do not start at 0", who); return false; }
        return true;
    }
    if (!stage_csr_ok(who, (int32_t)n_keys, key_off, err)) return false;
    if (key_off[n_keys] > STAGE_MAX) { err("%s: index: more than 2^30 - 1 positions", who); return false; }
    if (key_off[n_keys] > 0 && !pos) { err("%s: index: k outside 1 .. 28, no target, a key count outside 0 .. 2^30 - 1 or an array missing", who); return false; }
    const uint64_t hmask = ((uint64_t)1 << 2 * k) - 1;
    for (int64_t i = 0; i < n_keys; ++i)
        if (keys[i] > hmask || (i > 0 && keys[i] <= keys[i - 1])) { err("%s: index: key %lld: not ascending, or outside 2k bits", who, (long long)i); return false; }
    for (int64_t i = 0; i < key_off[n_keys]; ++i) {
        const uint64_t rid = pos[i] >> 32, p = (uint32_t)pos[i] >> 1;
        if (rid >= (uint64_t)n_seq || p >= (uint64_t)lens[rid]) { err("%s: index: position %lld: outside its target", who, (long long)i); return false; }
    }
    return true;
}

// The minimizers of n reads by mz_off, in the sketch's layout (x = hash << 8 | span, low half of y = last_pos << 1 | strand): the
// hash inside 2k bits (the lookup's bucket table ends there), 1 <= span <= min(255, last_pos + 1), last_pos < seq_len and never
// decreasing inside a read (the rep_len scan of seed_prefix_kernel takes the interval ends as ascending).
inline bool stage_seed_mz_ok(const char *who, int32_t k, int32_t n, const int64_t *mz_off, const uint64_t *mz, const int32_t *seq_len, err_fn err) {
    if (n <= 0) return true;
    if (!mz_off || !seq_len) { err("%s: an array missing", who); return false; }
    if (!stage_csr_ok(who, n, mz_off, err)) return false;
    if (mz_off[n] > STAGE_MAX) { err("%s: more than 2^30 - 1 minimizers", who); return false; }
    if (mz_off[n] > 0 && !mz) { err("%s: an array missing", who); return false; }
    const uint64_t hmask = ((uint64_t)1 << 2 * k) - 1;
    for (int32_t i = 0; i < n; ++i) {
        if (seq_len[i] < 0) { err("%s: read %d: negative length", who, i); return false; }
        int64_t prev = -1;
        for (int64_t m = mz_off[i]; m < mz_off[i + 1]; ++m) {
            const uint64_t x = mz[2 * m];
            const int64_t span = (int64_t)(x & 0xff), last = (int64_t)((uint32_t)mz[2 * m + 1] >> 1), j = m - mz_off[i];
            if (x >> 8 > hmask) { err("%s: read %d: minimizer %lld: hash outside 2k bits", who, i, (long long)j); return false; }
            if (span < 1 || span > last + 1) { err("%s: read %d: minimizer %lld: span outside 1 .. min(255, last_pos + 1)", who, i, (long long)j); return false; }
            if (last >= seq_len[i]) { err("%s: read %d: minimizer %lld: last_pos outside the read", who, i, (long long)j); return false; }
            if (last < prev) { err("%s: read %d: minimizer %lld: last_pos decreases", who, i, (long long)j); return false; }
            prev = last;
        }
    }
    return true;
}

// the options the seed half reads and the tests' knobs (max_gap's upper end is the library's chain_gap_check)
inline bool stage_seed_knobs_ok(const char *who, int32_t mid_occ, int32_t min_cnt, int32_t max_gap, int64_t flt_round2, int32_t flt_wgs,
                                int32_t grid_cap, int64_t cap, err_fn err) {
    if (mid_occ < 1 || mid_occ > (1 << 25)) { err("%s: mid_occ %d outside 1 .. 2^25", who, mid_occ); return false; }
    if (min_cnt < 0 || max_gap < 0) { err("%s: a negative option", who); return false; }
    if (flt_round2 < 0 || flt_wgs < 0 || grid_cap < 0 || cap < 0) { err("%s: flt_round2, flt_wgs, grid_cap or the capacity negative", who); return false; }
    return true;
}

// n (query, target) pairs of 0..4 codes, checked, with the buffers the kernels read.  The arrays of the caller are kept by pointer.
struct StagePairs {
    int32_t n = 0;
    const int64_t *q_off = nullptr, *t_off = nullptr, *cig_off = nullptr;
    const int32_t *q_len = nullptr, *t_len = nullptr, *n_cigar = nullptr;
    const uint8_t *tcodes = nullptr;           // [0, ttot): for pack_2bit, which the library has and this header has not
    int64_t qtot = 0, ttot = 0, ctot = 0;      // the ends of the last query, target and CIGAR
    std::vector<int32_t> qspan, tspan;         // per pair: the bases its CIGAR consumes (with a CIGAR)
    std::vector<uint8_t> reads;                // ASCII, ((qtot + 19) & ~3) bytes, 'N' behind the last base
    std::vector<uint32_t> cigar;               // ctot ops and a 0 behind them (with a CIGAR)
};

// Everything is checked here, before any launch: lengths and intervals inside the sequences, offsets in 0 .. STAGE_MAX (an entry
// is given no buffer sizes: the end of the last pair is taken for the size, so a larger offset cannot be told from a larger
// buffer, only an absurd one), only M/I/D ops (an empty one only with allow_empty_ops), a CIGAR that consumes exactly
// [qs, qe) and stays inside the target.  qs/qe/ts and cigar/cig_off/n_cigar are given together, or n_cigar is NULL and none is read.
inline bool stage_pairs_build(const char *who, int32_t n, const uint8_t *qcodes, const int64_t *q_off, const int32_t *q_len,
                              const uint8_t *tcodes, const int64_t *t_off, const int32_t *t_len, const int32_t *qs, const int32_t *qe,
                              const int32_t *ts, const uint32_t *cigar, const int64_t *cig_off, const int32_t *n_cigar,
                              bool allow_empty_ops, err_fn err, StagePairs &sp) {
    sp = StagePairs();
    sp.n = n; sp.q_off = q_off; sp.q_len = q_len; sp.t_off = t_off; sp.t_len = t_len; sp.cig_off = cig_off; sp.n_cigar = n_cigar;
    sp.tcodes = tcodes;
    if (n_cigar) { sp.qspan.resize((size_t)n); sp.tspan.resize((size_t)n); }
    for (int i = 0; i < n; ++i) {
        if (q_len[i] < 0 || t_len[i] < 0 ||
            (n_cigar && (n_cigar[i] < 0 || qs[i] < 0 || qe[i] < qs[i] || qe[i] > q_len[i] || ts[i] < 0 || ts[i] > t_len[i] || cig_off[i] < 0))) {
            err("%s: pair %d: intervals outside the sequences", who, i); return false;
        }
        if (q_off[i] < 0 || q_off[i] > STAGE_MAX - q_len[i] || t_off[i] < 0 || t_off[i] > STAGE_MAX - t_len[i] ||
            (n_cigar && cig_off[i] > STAGE_MAX - n_cigar[i])) {
            err("%s: pair %d: an offset negative, or an end beyond 2^30 - 1", who, i); return false;
        }
        if (q_off[i] + q_len[i] > sp.qtot) sp.qtot = q_off[i] + q_len[i];
        if (t_off[i] + t_len[i] > sp.ttot) sp.ttot = t_off[i] + t_len[i];
        if (!n_cigar) continue;
        int64_t ql = 0, tl = 0;
        for (int k = 0; k < n_cigar[i]; ++k) {
            const uint32_t c = cigar[cig_off[i] + k], op = c & 0xf, len = c >> 4;
            if (op > 2 || (len == 0 && !allow_empty_ops)) {
                err(allow_empty_ops ? "%s: pair %d: op %d is not M, I or D" : "%s: pair %d: op %d is not a non-empty M, I or D", who, i, k); return false;
            }
            ql += op != 2 ? len : 0; tl += op != 1 ? len : 0;
        }
        if (ql != qe[i] - qs[i] || ts[i] + tl > t_len[i]) { err("%s: pair %d: the CIGAR does not consume its read interval or leaves the target", who, i); return false; }
        if (cig_off[i] + n_cigar[i] > sp.ctot) sp.ctot = cig_off[i] + n_cigar[i];
        sp.qspan[(size_t)i] = (int32_t)ql; sp.tspan[(size_t)i] = (int32_t)tl;
    }
    sp.reads.assign(((size_t)sp.qtot + 19) & ~(size_t)3, 'N');
    for (int64_t i = 0; i < sp.qtot; ++i) sp.reads[(size_t)i] = (uint8_t)"ACGTN"[qcodes[i] > 4 ? 4 : qcodes[i]];
    if (n_cigar) { sp.cigar.assign(cigar, cigar + sp.ctot); sp.cigar.push_back(0); }
    return true;
}

}  // namespace mpn_stage
