// The walk over BAM text behind mpn_bam_walk (include/mpn_ingest.h), written from the SAM/BAM specification section 4.2.  It
// compiles for the device (csrc/bam_in_kernels.hip) and for the host (scripts/bam_walk_host_check.cpp runs every test case,
// malformed ones included, through it under the sanitizers).
//
// The text is the inflated BAM stream from `start` on: first the header (magic, l_text, text, n_ref, the reference entries), then
// records chained through their block_size fields.  Three pieces, so that the kernel can do the chain with one lane and the rows
// with all of them:
//   bamw_header   the whole header -> the offset of the first record
//   bamw_step     the 4 bytes of block_size at a record start -> whether the record is whole, partial or malformed
//   bamw_row      the 32 fixed bytes of a whole record -> its table row, or malformed
// bamw_walk_serial is the three together on one thread.  Bounds: every read is of text[a .. a + k) with a + k <= len checked in
// 64-bit arithmetic right before it; bamw_row is only called for records that bamw_step found whole and of 32 bytes at least.
#pragma once
#include <stdint.h>
#include "../../include/mpn_ingest.h"

#if defined(__HIPCC__)
#define BAMW_HD __host__ __device__ inline
#else
#define BAMW_HD inline
#endif

namespace mpn_bamw {

enum { BAMW_WHOLE = 0, BAMW_END = 1, BAMW_PARTIAL = 2, BAMW_BAD = 3 };

constexpr int BAMW_FIXED = 36;          // block_size and the 32 fixed bytes behind it

BAMW_HD uint32_t bamw_u16(const uint8_t *t, int64_t a) { return (uint32_t)t[a] | ((uint32_t)t[a + 1] << 8); }
BAMW_HD int32_t bamw_i32(const uint8_t *t, int64_t a) {
    return (int32_t)((uint32_t)t[a] | ((uint32_t)t[a + 1] << 8) | ((uint32_t)t[a + 2] << 16) | ((uint32_t)t[a + 3] << 24));
}

// The header at text[start ..): BAMW_WHOLE and *next = the first record's offset; BAMW_PARTIAL: it passes the end of the text
// (*next = start); BAMW_BAD with *status = MPN_BAM_BAD_MAGIC or MPN_BAM_BAD_HEADER.  At most (len - start) / 5 steps.
BAMW_HD int bamw_header(const uint8_t *t, int64_t len, int64_t start, int64_t *next, int32_t *status) {
    *next = start;
    const int64_t have = len - start;
    // the magic is judged on the bytes that are there: a file that is no BAM is refused before its l_text is believed
    for (int k = 0; k < 4 && k < have; ++k)
        if (t[start + k] != ((0x014d4142u >> (8 * k)) & 0xffu)) { *status = MPN_BAM_BAD_MAGIC; return BAMW_BAD; }      // B A M \1
    if (have < 8) return BAMW_PARTIAL;
    const int32_t l_text = bamw_i32(t, start + 4);
    if (l_text < 0) { *status = MPN_BAM_BAD_HEADER; return BAMW_BAD; }
    int64_t p = start + 8 + (int64_t)l_text;
    if (p + 4 > len) return BAMW_PARTIAL;
    const int32_t n_ref = bamw_i32(t, p);
    if (n_ref < 0) { *status = MPN_BAM_BAD_HEADER; return BAMW_BAD; }
    p += 4;
    for (int32_t r = 0; r < n_ref; ++r) {
        if (p + 4 > len) return BAMW_PARTIAL;
        const int32_t l_name = bamw_i32(t, p);
        if (l_name < 1) { *status = MPN_BAM_BAD_HEADER; return BAMW_BAD; }
        p += 4 + (int64_t)l_name + 4;        // the name and l_ref
        if (p > len) return BAMW_PARTIAL;
    }
    *next = p;
    return BAMW_WHOLE;
}

// The record that starts at text[off]: BAMW_END (off is the end of the text), BAMW_PARTIAL (it passes the end), BAMW_BAD
// (block_size < 32), or BAMW_WHOLE with *end = the next record's offset.
BAMW_HD int bamw_step(const uint8_t *t, int64_t len, int64_t off, int64_t *end) {
    if (off >= len) return BAMW_END;
    if (off + 4 > len) return BAMW_PARTIAL;
    const int32_t block_size = bamw_i32(t, off);
    if (block_size < 32) return BAMW_BAD;
    *end = off + 4 + (int64_t)block_size;
    return *end > len ? BAMW_PARTIAL : BAMW_WHOLE;
}

// The row of the whole record text[off .. end), end - off >= 36.  Returns 0, or 1 for a record whose lengths do not fit into it.
// has_qual: the quality field exists and its first byte is not 0xFF (a record without bases has no such byte: 0).
BAMW_HD int bamw_row(const uint8_t *t, int64_t off, int64_t end, mpn_bam_row *row) {
    const int64_t block_size = end - off - 4;
    const int32_t l_read_name = t[off + 12];
    const int64_t n_cigar = bamw_u16(t, off + 16);
    const uint32_t flag = bamw_u16(t, off + 18);
    const int32_t l_seq = bamw_i32(t, off + 20);
    if (l_read_name < 1 || l_seq < 0) return 1;
    const int64_t qual = 32 + (int64_t)l_read_name + 4 * n_cigar + ((int64_t)l_seq + 1) / 2;
    if (qual + l_seq > block_size) return 1;
    row->off = off;
    row->l_seq = l_seq;
    row->flag = (uint16_t)flag;
    row->l_read_name = (uint8_t)l_read_name;
    row->has_qual = (uint8_t)(l_seq > 0 && t[off + 4 + qual] != 0xFF);
    return 0;
}

// Where the packed bases of a row's record start in the text (the qualities follow them at + (l_seq + 1) / 2).
BAMW_HD int64_t bamw_seq_off(const uint8_t *t, const mpn_bam_row *row) {
    return row->off + BAMW_FIXED + (int64_t)row->l_read_name + 4 * (int64_t)bamw_u16(t, row->off + 16);
}

// The whole walk on one thread: mpn_bam_walk's contract (include/mpn_ingest.h).
BAMW_HD void bamw_walk_serial(const uint8_t *t, int64_t len, int64_t start, int at_header, int final_call, int64_t max_records,
                              mpn_bam_row *rows, int64_t *n_records, int64_t *next, int32_t *status) {
    *n_records = 0; *next = start; *status = MPN_INFLATE_OK;
    int64_t off = start;
    if (at_header) {
        const int h = bamw_header(t, len, start, &off, status);
        if (h == BAMW_BAD) return;
        if (h == BAMW_PARTIAL) { if (final_call) *status = MPN_BAM_TRUNCATED; return; }
        *next = off;
    }
    int64_t n = 0;
    while (n < max_records) {
        int64_t end = 0;
        const int s = bamw_step(t, len, off, &end);
        if (s == BAMW_END) break;
        if (s == BAMW_PARTIAL) { if (final_call) *status = MPN_BAM_TRUNCATED; break; }
        if (s == BAMW_BAD || bamw_row(t, off, end, rows + n)) { *status = MPN_BAM_BAD_RECORD; break; }
        ++n;
        off = end;
    }
    *n_records = n;
    *next = off;
}

}  // namespace mpn_bamw
