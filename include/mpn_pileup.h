/*
 * mpn_pileup.h -- C-ABI of the per-base pile-up of a sorted BAM on the GPU (csrc/pileup_kernels.hip) and of the candidate sites
 * Clair's preprocess/ExtractVariantCandidates.py makes of it (megapath_nano_amd/candidates.py; the rules are DESIGN.md section 6).
 * The BAM text is resident: mpn_gzip_inflate_device, mpn_bam_flatten and mpn_bam_walk (mpn_ingest.h) have put it there and found
 * its records.
 *
 *   mpn_pileup_records     the rows of mpn_bam_walk -> what the fixed fields and the CIGAR of every record say
 *   mpn_pileup_counts      the taken records, sorted by position -> seven int32 counters per position of a window, in HBM
 *   mpn_pileup_candidates  the counters, the reference bytes and the thresholds -> the table of the positions that pass, in order
 *
 * The per-record CIGAR arithmetic and the per-position decision are csrc/pileup_core.h, which also compiles for the host
 * (scripts/pileup_host_check.cpp runs the whole pile-up serially through it).  Calling rules as in mpn_ingest.h: a call returns
 * when its results are on the host, the default stream is used, 0 = done, -1 = device error (mpn_last_error()), -2 = bad
 * arguments, -3 = a capacity is too small.  Malformed records end in a status, never in an access outside the text.
 */
#ifndef MPN_PILEUP_H
#define MPN_PILEUP_H
#include <stdint.h>
#include "mpn_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The counters of a position, in this order; a candidate line starts from it. */
#define MPN_PILEUP_SLOTS 7          /* A C G T I D N */
#define MPN_PILEUP_TILE 2048        /* positions a workgroup of mpn_pileup_counts owns: 7 x 4 B x 2048 = 56 KiB of LDS */
#define MPN_PILEUP_SLICE 128        /* records of a tile one workgroup takes; a tile with more is split over several (measured: profiles/r20_candidates) */

enum {
    MPN_PILEUP_OK = 0,
    MPN_PILEUP_CIGAR_PAST = 1,      /* the CIGAR, or the packed bases behind it, pass the end of the record or of the text */
    MPN_PILEUP_BAD_OP = 2,          /* an operation code above 8 */
    MPN_PILEUP_PLACEHOLDER = 3,     /* <l_seq>S<n>N: the real CIGAR is in a CG tag (more than 65535 operations) */
    MPN_PILEUP_NO_BASE = 4          /* an M, = or X operation reaches past l_seq (a record without bases among them) */
};

/* What a record says.  Operations: M I D N S H P = X are 0 .. 8.  soft: the summed length of S; total: of all operations;
 * span: of M, =, X and D -- N does NOT advance the reference here, as in the reference script. */
typedef struct {
    int64_t soft, total, span;
    int32_t ref_id, pos;
    uint16_t n_cigar;
    uint8_t mapq, status;
    int32_t reserved;
} mpn_pileup_rec;

/* recs[r] (host, n entries) for the record at rows[r].off of d_text[0 .. text_len) (DEVICE pointer; rows: host, of mpn_bam_walk on
 * this text).  A lane per record.  -2 before anything is launched for a row whose 36 fixed bytes do not lie inside the text. */
int32_t mpn_pileup_records(const void *d_text, int64_t text_len, int64_t n, const mpn_bam_row *rows, mpn_pileup_rec *recs);

/* A taken record: where it starts in the text, its position, and whether an I or D that occurs while the reference position is
 * still pos counts (at pos - 1).  The caller decides that: the first taken record of its pos. */
typedef struct {
    int64_t off;
    int32_t pos;
    int32_t lead;
} mpn_pileup_take;

/* Adds the counts of n taken records (host; ascending pos, -2 otherwise; span[r]: of mpn_pileup_records) inside the window
 * [lo, hi) of the contig to d_counts (DEVICE, int32, MPN_PILEUP_SLOTS per position, position p at (p - lo) * 7): the caller zeroes
 * it before the first call and may call once per text of a file.  M, = and X add one to the slot of the read base per base
 * (4-bit codes: M R W V H D -> A, S Y B -> C, K -> G, N -> N); I and D add one to their slot at the position before them; S
 * advances the read; H, P and N do nothing.
 * A workgroup owns a tile of MPN_PILEUP_TILE positions and the records that can reach it, a wave one record at a time; counts go
 * to the tile in LDS by LDS atomics.  A tile with more than `slice` records (0: MPN_PILEUP_SLICE) is split over several
 * workgroups, which add their tiles to d_counts by atomic adds; a tile with one workgroup adds without atomics.  All sums are
 * integers: the result is the same bit for bit from run to run.  *n_sliced (or NULL): the tiles that were split.
 * *bad_row: -1, or the smallest r whose record has code 0 ('=') or no base under an M, = or X, or does not lie inside the
 * text; the counters are not to be used then. */
int32_t mpn_pileup_counts(const void *d_text, int64_t text_len, int64_t n, const mpn_pileup_take *takes, const int64_t *span, int64_t lo,
                          int64_t hi, int32_t slice, void *d_counts, int64_t *bad_row, int64_t *n_sliced);

/* A row of the table: the 0-based position, the mapped reference base, the depth A + C + G + T + N, and the seven counts in
 * stable descending order with the letter of each. */
typedef struct {
    int32_t pos, depth;
    int32_t count[MPN_PILEUP_SLOTS];
    uint8_t label[MPN_PILEUP_SLOTS];
    uint8_t ref_base;
} mpn_pileup_cand;

/* The positions of [lo, lo + n_pos) that pass, ascending, to rows[0 .. *n_rows) (host, cap entries; -3 with *n_rows complete if
 * cap is too small).  ref (host, n_pos bytes): the reference byte of every position, 0 where the sequence has none.  A position
 * passes when it has any count, lies in one of the n_bed intervals [bed_start[i], bed_end[i]) (host; sorted and disjoint; n_bed
 * < 0: no BED), its reference byte is one of ACGTURYSWKMBDHVN, (double)depth >= min_coverage, and the top label is not the
 * reference base or (double)second / (double)depth >= threshold.  Decided per position on the device in float64; compacted with a
 * scan, so that the order is the position order.  The counters stay in HBM. */
int32_t mpn_pileup_candidates(const void *d_counts, int64_t lo, int64_t n_pos, const uint8_t *ref, int64_t n_bed, const int64_t *bed_start,
                              const int64_t *bed_end, double min_coverage, double threshold, int64_t cap, mpn_pileup_cand *rows,
                              int64_t *n_rows);

/* Device time of the calling thread's last call of each of the three, in milliseconds.  Any pointer may be NULL. */
void mpn_pileup_last_device_ms(double *records_ms, double *counts_ms, double *candidates_ms);

#ifdef __cplusplus
}
#endif
#endif
