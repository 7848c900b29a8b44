/*
 * mpn_tensor.h -- C-ABI of Clair's input tensors built on the GPU from candidate sites (csrc/tensor_kernels.hip), the drop-in for
 * preprocess/CreateTensor.py (megapath_nano_amd/clair_tensor.py; the rules are DESIGN.md section 6).  The BAM text is resident, as
 * for mpn_pileup.h, and so are the bytes of the reference sequence.
 *
 *   mpn_tensor_records       the rows of mpn_bam_walk -> what mpn_pileup_rec does not say: htslib's reference length, bases, qualities
 *   mpn_tensor_join          taken records and sorted centres -> the records that join every centre, a CSR pair list in HBM
 *   mpn_tensor_centre_flags  pairs of deep centres -> one byte per pair: the read has a high-quality base at the centre
 *   mpn_tensor_fill          a list of reads per tensor -> 33 x 8 x 4 int32 per tensor in HBM, and the depth at its centre
 *   mpn_tensor_emit          kept tensors -> the text of the reference's lines, in HBM
 *
 * The arithmetic shared by host and device is csrc/tensor_core.h (scripts/tensor_host_check.cpp runs it serially).  Calling rules
 * as in mpn_pileup.h: a call returns when its results are on the host, the default stream is used, 0 = done, -1 = device error
 * (mpn_last_error()), -2 = bad arguments, -3 = a capacity is too small.  Malformed records end in a status or in *bad_read, never
 * in an access outside the text.  A centre is always given 0-based (c0 = the 1-based candidate position - 1).
 */
#ifndef MPN_TENSOR_H
#define MPN_TENSOR_H
#include <stdint.h>
#include "mpn_pileup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_TENSOR_FLANK 16         /* param.flankingBaseNum */
#define MPN_TENSOR_POSITIONS 33     /* 2 * flank + 1 */
#define MPN_TENSOR_ROWS 8           /* A C G T, forward then reverse strand */
#define MPN_TENSOR_CHANNELS 4
#define MPN_TENSOR_CELLS 1056       /* 33 x 8 x 4 */
#define MPN_TENSOR_DEPTH 100        /* reads of one tensor at the most (matrix_depth) */
#define MPN_TENSOR_QUAL 7           /* raw quality from which a centre base is a high-quality one */

/* What a record says beyond mpn_pileup_rec.  hts_len: the summed length of M, D, N, = and X (htslib's bam_endpos counts N; a
 * record of length 0 ends one base behind its pos: the caller's rule).  has_qual: l_seq > 0 and the first quality byte is not
 * 0xff.  status: MPN_PILEUP_OK, _CIGAR_PAST (the CIGAR, the bases or the qualities pass the end of the record or of the text),
 * _BAD_OP, _NO_BASE. */
typedef struct {
    int64_t hts_len;
    int32_t l_seq;
    uint8_t has_qual, status;
    uint16_t reserved;
} mpn_tensor_rec;

/* recs[r] (host) for the record at rows[r].off of d_text (DEVICE).  A lane per record.  -2 for a row outside the text. */
int32_t mpn_tensor_records(const void *d_text, int64_t text_len, int64_t n, const mpn_bam_row *rows, mpn_tensor_rec *recs);

/* The join.  pos[r], span[r] (host, n taken records in file order, pos ascending, span of mpn_pileup_records: M, =, X and D) and
 * the m centres c0[c] (host, strictly ascending).  A record joins a centre if it has an M, =, X or D at a position of
 * [c0 - 16, c0 + 17] (left_edge != 0), or at exactly c0 - 16 (left_edge == 0).  begin[c], end[c] (host): the range of records that
 * is looked at for centre c; the caller finds it by bisection.  A wave per centre: ballot, count, and a stable compaction.
 * d_pairs == NULL: counts[c] (host) = the records that join.  Otherwise the record indices of centre c are written, in file
 * order, to ((int32_t *)d_pairs)[pair_off[c] ..] (DEVICE, pairs_cap entries; pair_off: host, the running sum of the counts) and
 * counts is filled again. */
int32_t mpn_tensor_join(int64_t n, const int32_t *pos, const int64_t *span, int64_t m, const int32_t *c0, const int64_t *begin,
                        const int64_t *end, int32_t left_edge, int64_t *counts, const int64_t *pair_off, void *d_pairs, int64_t pairs_cap);

/* A taken record for the kernels that read its text. */
typedef struct {
    int64_t off;
    int32_t pos;
    int32_t reverse;       /* FLAG & 16 */
} mpn_tensor_read;

/* flags[i] (host, n_f bytes) = 1 if the read ((int32_t *)d_pairs)[pair[i]] has a high-quality base at the centre c0[i] (host
 * arrays of n_f entries): an M, = or X there with a raw quality of at least MPN_TENSOR_QUAL, or a D that covers it and that the
 * reference script records (not the D at which the read joins).  A wave per entry.  *bad_read: -1 or the smallest index of a read
 * that does not lie inside the text or has no base there. */
int32_t mpn_tensor_centre_flags(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_tensor_read *reads, const void *d_pairs,
                                int64_t n_pairs, int64_t n_f, const int64_t *pair, const int32_t *c0, int32_t left_edge, uint8_t *flags,
                                int64_t *bad_read);

/* One tensor: its centre and its n <= MPN_TENSOR_DEPTH reads: the pairs begin .. begin + n (via_sel == 0), or the pairs
 * sel[begin .. begin + n) (via_sel != 0). */
typedef struct {
    int64_t begin;
    int32_t c0;
    int32_t n;
    int32_t via_sel;
    int32_t reserved;
} mpn_tensor_job;

/* Fills n_jobs tensors: d_tensors (DEVICE, int32, MPN_TENSOR_CELLS per job, cell ((index * 8 + row) * 4 + channel)), depth[j]
 * (host) = the sum over the eight rows of channel 0 at index 16.  d_ref (DEVICE): the ref_len bytes of the reference sequence
 * from the 0-based position ref_start on.  sel (host, n_sel pair indices) may be NULL when no job goes through it.  A workgroup
 * per tensor, the tile in LDS, a wave per read; integer sums only.  *bad_read: -1, or the smallest index of a read that does not
 * lie inside the text, has an operation code above 8, no base under an M, = , X or I that counts, or that reaches a position of
 * the window outside the reference bytes; the tensors are not to be used then. */
int32_t mpn_tensor_fill(const void *d_text, int64_t text_len, int64_t n_reads, const mpn_tensor_read *reads, const void *d_pairs, int64_t n_pairs,
                        int64_t n_sel, const int64_t *sel, int64_t n_jobs, const mpn_tensor_job *jobs, int32_t left_edge, const void *d_ref,
                        int64_t ref_start, int64_t ref_len, void *d_tensors, int32_t *depth, int64_t *bad_read);

/* One line: the tensor it prints, its 1-based centre, and the slice of the reference bytes it shows. */
typedef struct {
    int64_t tensor;
    int64_t ref_off;
    int32_t ref_n;
    int32_t centre;
} mpn_tensor_line;

/* The lines `name centre refseq t0 .. t1055\n`.  d_out == NULL: line_len[i] (host) = the bytes of line i, by a block reduction per
 * line.  Otherwise the lines are written to d_out (DEVICE, out_cap bytes) at line_off[i] (host; the running sum of the lengths),
 * a block per line, the place of every number by a block scan.  -3 if a line would pass out_cap. */
int32_t mpn_tensor_emit(const void *d_tensors, int64_t n_tensors, int64_t n_lines, const mpn_tensor_line *lines, const void *d_ref, int64_t ref_len,
                        const char *name, int32_t name_len, int64_t *line_len, const int64_t *line_off, void *d_out, int64_t out_cap);

/* Device time of the calling thread's last call of join, centre_flags, fill and emit, in milliseconds.  Any pointer may be NULL. */
void mpn_tensor_last_device_ms(double *join_ms, double *flags_ms, double *fill_ms, double *emit_ms);

#ifdef __cplusplus
}
#endif
#endif
