/*
 * mpn_read_realign.h -- C-ABI of the parts of realignment/realign_illumina_reads.py that run over every base of every read and over
 * every read of every window (csrc/read_realign_kernels.hip; megapath_nano_amd/read_realign.py is the script itself; the rules
 * are DESIGN.md section 6).  The BAM text is resident, as for mpn_pileup.h, and so are the upper-cased bytes of the contig.
 *
 *   mpn_rr_records   the rows of mpn_bam_walk -> what the script reads from a `samtools view` line
 *   mpn_rr_chunks    the script's chunk recurrence over the positions of the viewed records (host only: a serial recurrence)
 *   mpn_rr_support   the counted records -> pileup[...]["X"] at the 5041 positions the script looks at on each yield, in HBM
 *   mpn_rr_assign    find_max_overlap_index over all member reads for the windows of every split of a chunk -> a CSR of reads
 *
 * The per-record arithmetic, the recurrence, the counting rules and the overlap rule are csrc/read_realign_core.h, which also
 * compiles for the host (scripts/read_realign_host_check.cpp runs all four serially through it).  Calling rules as in
 * mpn_pileup.h: a call returns when its results are where it says, the default stream is used, 0 = done, -1 = device error
 * (mpn_last_error()), -2 = bad arguments.  Malformed records end in a status, never in an access outside the text.
 */
#ifndef MPN_READ_REALIGN_H
#define MPN_READ_REALIGN_H
#include <stdint.h>
#include "mpn_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_RR_CHUNK 5000           /* realign_chunk_size */
#define MPN_RR_EXPAND 20            /* region_expansion_in_bp */
#define MPN_RR_ROW 5041             /* chunk_start - 21 .. chunk_end + 19: the positions a yield looks at */
#define MPN_RR_MIN_MQ 20            /* min_dbg_mapping_quality: records below it count nothing */
#define MPN_RR_MIN_BQ 20            /* min_dbg_base_quality */
#define MPN_RR_SLICE 256            /* records of a row one workgroup takes; a row with more is split over several */

enum {
    MPN_RR_OK = 0,
    MPN_RR_PAST = 1,                /* the CIGAR, the bases, the qualities or an aux field pass the end of the record or of the text */
    MPN_RR_BAD_OP = 2,              /* an operation code above 8 */
    MPN_RR_PLACEHOLDER = 3,         /* <l_seq>S<n>N: the real CIGAR is in a CG tag */
    MPN_RR_BAD_AUX = 4,             /* an aux field of a type other than A c C s S i I f Z H B, or a B array of another subtype */
    MPN_RR_HP_TEXT = 5,             /* a Z or H value holds the text `HP:i:`: the script would take it for the tag */
    MPN_RR_BASE_EQ = 6,             /* a base `=` (4-bit code 0) */
    MPN_RR_NO_BASE = 7              /* the operations that take bases take more than l_seq */
};

/* What a record says.  soft: the summed length of S; total: of all operations; del: of D; span: of M, =, X and D (N does not move
 * the script's reference position).  The script's read_end is pos + l_seq + del.  hp: the character the script keeps of the first
 * aux field HP of an integer type (c C s S i I): the first character of its decimal value if that is a digit, else 0.  clipped: the
 * script's soft-clip test holds, 1.0 - soft / (total + 1) < 0.55 in float64: the record is dropped.  status is
 * the first of the list above that holds, in the order PAST, BAD_OP, PLACEHOLDER, NO_BASE, BASE_EQ, BAD_AUX, HP_TEXT. */
typedef struct {
    int64_t soft, total, del, span;
    int32_t ref_id, pos, l_seq, next_ref, next_pos;
    uint16_t flag, n_cigar;
    uint8_t mapq, has_seq, has_qual, hp, status, clipped, reserved[2];
} mpn_rr_rec;

/* recs[r] (host, n entries) for the record at rows[r].off of d_text[0 .. text_len) (DEVICE; rows: host, of mpn_bam_walk on this
 * text).  A lane per record.  -2 before anything is launched for a row whose 36 fixed bytes do not lie inside the text. */
int32_t mpn_rr_records(const void *d_text, int64_t text_len, int64_t n, const mpn_bam_row *rows, mpn_rr_rec *recs);

/* The chunk recurrence (host only).  pos[i]: the 0-based POS of the viewed records of the contig in file order, dropped ones
 * included.  *first (in, out): the first record's POS, -1 before the first call; *chunk (in, out): the number of yields so far.
 * chunk_of[i]: the chunk that is current when the script parses record i, after the yield the record may trigger -- its
 * chunk_start is *first + 5000 * chunk_of[i].  A record with POS >= chunk_end + 20 triggers one yield and moves the chunk on
 * once, however far ahead it is.  May be called once per text. */
int32_t mpn_rr_chunks(int64_t n, const int32_t *pos, int64_t *first, int64_t *chunk, int32_t *chunk_of);

/* A counted record: where it starts in the text, its position, the chunk_start that is current when the script parses it, and
 * the number of that chunk. */
typedef struct {
    int64_t off;
    int32_t pos, chunk_start, chunk, reserved;
} mpn_rr_take;

/* Adds to d_rows (DEVICE, int32, MPN_RR_ROW per epoch; the caller zeroes it, and may call once per text) the counts of the n
 * taken records (host; pos and chunk ascending, -2 otherwise; reach[r] = l_seq + span of mpn_rr_records).  Epoch e (host arrays of
 * n_epochs entries) is the yield of chunk epoch_chunk[e] (strictly ascending): its row holds positions row_lo[e] .. + 5040 and
 * takes the records whose chunk is at most epoch_chunk[e].  d_contig[0 .. contig_len): DEVICE, the upper-cased contig.  Rules
 * (csrc/read_realign_core.h): only records with MAPQ >= 20 count; `=` moves both positions; M and X count a base of quality >= 20
 * over a contig base of ACGT that differs from the read's letter; I and S at p add one to [p - len, p + len) if p lies inside
 * [chunk_start - 20, chunk_start + 5020] of the record's own chunk, the base before p (the contig's last at p = 0) is one of ACGT
 * and all len qualities are >= 20; D adds one to [p, p + len) under the first two and moves on; N, H and P do nothing.
 * A workgroup takes one row and a slice of at most `slice` (0: MPN_RR_SLICE) of the records that can reach it (bisected on the
 * host: pos - l_seq .. pos + span + l_seq), with the row in LDS, a wave per record, 64 operations a step.  A row with one
 * workgroup is stored plainly, a row split over several is added with atomicAdd.  Integer sums: bit-identical from run to run.
 * *bad_row: -1, or the smallest r whose record does not lie inside the text, has an operation code above 8, needs a base or
 * quality it does not have, or needs a contig base at or behind contig_len; the rows are not to be used then.  *n_split (or
 * NULL): the rows that were split. */
int32_t mpn_rr_support(const void *d_text, int64_t text_len, int64_t n, const mpn_rr_take *takes, const int64_t *reach, int64_t n_epochs,
                       const int32_t *epoch_chunk, const int32_t *row_lo, const void *d_contig, int64_t contig_len, int32_t slice, void *d_rows,
                       int64_t *bad_row, int64_t *n_split);

/* find_max_overlap_index for n member reads (host; pos[r], end[r] = the script's read_start and read_end, in member order) against
 * the windows of n_splits splits: split s has the windows win_begin[s] .. win_begin[s + 1] of win_start / win_end (host; sorted and
 * disjoint within a split, -2 otherwise).  A read goes to the window of its split with the largest
 * min(end, win_end) - max(pos, win_start), to the first of them on a tie, and to none when that is not positive or pos is above the
 * split's largest win_end.  count[w] (host): the reads of window w; list (host, cap entries): the reads of window 0 in member
 * order, then those of window 1, ...; -3 if cap is too small (count is complete).  A lane per (split, read); the counts come to the
 * host, which sums them into the windows' offsets; then a workgroup per window that has reads compacts them in order with ballots
 * and prefix counts. */
int32_t mpn_rr_assign(int64_t n, const int32_t *pos, const int32_t *end, int32_t n_splits, const int32_t *win_begin, const int32_t *win_start,
                      const int32_t *win_end, int32_t *count, int32_t *list, int64_t cap);

/* Device time of the calling thread's last call of each of the three device calls, in milliseconds.  Any pointer may be NULL. */
void mpn_rr_last_device_ms(double *records_ms, double *support_ms, double *assign_ms);

#ifdef __cplusplus
}
#endif
#endif
